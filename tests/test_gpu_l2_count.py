"""Ratio-test counts per pair on SIFT rows, decided on the device (lcm_l2_count.hip / lcm_l2.cpp): lcm_score_pairs_ratio_l2,
lcm_loop_search_ratio_l2 and the diagnostic lcm_l2_ratio_test_device against tests/l2ref.py (knn2 + ratio_filter for the
count, distances_sq for the minimum) and the threshold formula of tests/l2countcases.py.  Needs a real MI355X.

LCM_TUNE_L2_COUNT_CHUNK (read on every call) pins the query chunk to 128 or 256 rows, i.e. k_l2_count<1> or <2>; every
call asserts the workgroups that served it: sum over the pairs with two non-empty sides of ceil(query rows / chunk)."""
import ctypes as C

import numpy as np
import pytest

import l2cases as L
import l2countcases as K
import l2ref

pytestmark = pytest.mark.gpu

NQ = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 600)
NT = (1, 2, 31, 32, 33, 511, 512, 513, 1025)
RATIOS = (0.7, 0.75, 1.0, 1e30)
AUTO_LARGE_ITEMS = 1024


@pytest.fixture(params=(128, 256))
def chunk(request, monkeypatch):
    monkeypatch.setenv("LCM_TUNE_L2_COUNT_CHUNK", str(request.param))
    return request.param


@pytest.fixture
def auto(monkeypatch):
    monkeypatch.delenv("LCM_TUNE_L2_COUNT_CHUNK", raising=False)


def auto_chunk(frames, pairs):
    return 128 if K.workgroups(frames, pairs, 256) < AUTO_LARGE_ITEMS else 256


def score(matcher, ch, frames, pairs, ratio, msg=""):
    """score_pairs_ratio_l2 of the call, after checking the launch that served it."""
    got = matcher.score_pairs_ratio_l2(frames, pairs, ratio)
    assert got.dtype == K.SCORE_DTYPE and len(got) == len(pairs)
    live = [(a, b) for a, b in pairs if len(frames[a]) and len(frames[b])]
    if live:
        info = matcher.launch_info()
        assert info.workgroups == K.workgroups(frames, pairs, ch), (msg, ch, info.workgroups)
        assert info.route == 0 and info.pairs == len(live), msg
        assert info.distances == sum(len(frames[a]) * len(frames[b]) for a, b in live), msg
        assert info.kernel_ms > 0
    return got


def check(matcher, ch, frames, pairs, ratio, refs=None, msg=""):
    got = score(matcher, ch, frames, pairs, ratio, msg)
    want = K.ref_scores(frames, pairs, ratio, refs)
    np.testing.assert_array_equal(got["good_count"], want["good_count"], err_msg=f"{msg} good_count, ratio {ratio} chunk {ch}")
    np.testing.assert_array_equal(got["min_dist_sq"], want["min_dist_sq"], err_msg=f"{msg} min_dist_sq, ratio {ratio} chunk {ch}")
    return got


# ---- shapes -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shapes():
    """One pair of the largest shape; the reference of every (nq, nt) prefix is made once and shared by both chunk sizes."""
    rng = np.random.default_rng(2026)
    q, t = K.mixed(rng, max(NQ)), K.mixed(rng, max(NT))
    D = l2ref.distances_sq(q, t)
    L.ro(q, t, D)
    refs = {}

    def ref(nq, nt):
        if (nq, nt) not in refs:
            d = np.ascontiguousarray(D[:nq, :nt])
            refs[(nq, nt)] = (l2ref.knn2(q[:nq], t[:nt], d), int(d.min()))
        return refs[(nq, nt)]
    return q, t, ref


@pytest.mark.parametrize("nt", NT)
def test_shapes(matcher, shapes, chunk, nt):
    q, t, ref = shapes
    seen = set()
    for nq in NQ:
        for ratio in RATIOS:
            got = score(matcher, chunk, [q[:nq], t[:nt]], [(0, 1)], ratio, f"{nq} x {nt}")[0]
            want = K.ref_score(q[:nq], t[:nt], ratio, ref(nq, nt))
            assert (int(got["good_count"]), int(got["min_dist_sq"])) == want, (nq, nt, ratio, chunk)
            if nt == 1:
                assert got["good_count"] == 0 and got["min_dist_sq"] != K.NONE
            elif ratio == 1e30:
                assert got["good_count"] == nq - int((ref(nq, nt)[0][2][:, 1] == 0).sum())
            seen.add((ratio, 0 < int(got["good_count"]) < nq))
    if nt >= 511:
        assert (0.7, True) in seen and (0.75, True) in seen          # survivors AND failures: the inputs decide something


def test_empty_sides(matcher, chunk):
    rng = np.random.default_rng(1)
    q = K.mixed(rng, 40)
    frames = [q, q[:0], q[:7]]
    pairs = [(0, 1), (1, 0), (1, 1), (0, 2), (1, 2), (2, 1), (2, 0)]
    got = check(matcher, chunk, frames, pairs, 0.75)
    for k, (a, b) in enumerate(pairs):
        if 1 in (a, b):
            assert tuple(got[k]) == (0, K.NONE)
    only_empty = matcher.score_pairs_ratio_l2(frames, [(0, 1), (1, 1)], 0.7)
    assert [tuple(r) for r in only_empty] == [(0, K.NONE)] * 2
    assert len(matcher.score_pairs_ratio_l2(frames, [], 0.7)) == 0
    assert len(matcher.score_pairs_ratio_l2([], [], 0.7)) == 0


# ---- the padding trap, both sides -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", (33, 513, 1000))
def test_pad_train_rows_are_no_neighbours(matcher, chunk, nt):
    q, t = K.pad_train_case(nt)
    for ratio in (0.7, 0.75, 1.0):
        got = check(matcher, chunk, [q, t], [(0, 1)], ratio)
        assert tuple(got[0]) == (len(q), 0)


@pytest.mark.parametrize("nq", (1, 33, 129))
def test_pad_query_rows_do_not_count(matcher, chunk, nq):
    q, t = K.pad_query_case(nq)
    for ratio, want in ((0.7, 0), (0.75, 0), (1.0, 0), (1.5, nq)):
        got = check(matcher, chunk, [q, t], [(0, 1)], ratio)
        assert tuple(got[0]) == (want, 2)


# ---- equal keys meet in one running list ------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", K.EQUAL_KEY_ROWS)
@pytest.mark.parametrize("front", (False, True))
def test_equal_keys_are_first_and_second_neighbour(matcher, chunk, where, front):
    q, t, expect, dmin = K.equal_keys_case(where, front=where[1] + 9 if front else None)
    for ratio, n in expect.items():
        got = check(matcher, chunk, [q, t], [(0, 1)], ratio)
        assert tuple(got[0]) == (n, dmin), (ratio, where, front)


# ---- the verdict's boundary, through descriptors ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def boundary():
    return K.boundary_frames()


def test_boundary_of_the_verdict(matcher, chunk, boundary):
    frames, pairs, cases = boundary
    nq = len(frames[0])
    for ratio in K.BOUNDARY_RATIOS:
        sel = [k for k, c in enumerate(cases) if c.ratio == ratio]
        got = score(matcher, chunk, frames, [pairs[k] for k in sel], ratio)
        for g, k in zip(got, sel):
            c = cases[k]
            assert tuple(g) == (nq if c.passes else 0, c.D1), c
    first = L.collision_table()[0][0]
    k = next(k for k, c in enumerate(cases) if c.ratio == 1.0 and c.D2 == first + 1 and c.D1 == first)
    assert tuple(score(matcher, chunk, frames, [pairs[k]], 1.0)[0]) == (0, first)          # equal roots: not counted


# ---- the verdict over the whole range of D, through the diagnostic ----------------------------------------------------------

ALL_D = K.MAX_D + 1
assert ALL_D <= 1 << 23                        # one call per array


@pytest.mark.parametrize("ratio", (0.5, 0.7, 0.75, 1.0))
def test_verdict_over_the_whole_range(matcher, ratio):
    D2 = np.arange(ALL_D, dtype=np.uint32)
    t = K.threshold(D2, ratio)
    assert t.max() <= K.MAX_D
    for D1 in (np.clip(t - 1, 0, K.MAX_D).astype(np.uint32), np.clip(t, 0, K.MAX_D).astype(np.uint32)):
        got = matcher.l2_ratio_test_device(D1, D2, ratio)
        want = (D1.astype(np.int64) < t).astype(np.uint8)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (ratio, bad[:5], D1[bad[:5]], D2[bad[:5]])
    # t - 1 passes wherever something passes, t never does
    assert matcher.l2_ratio_test_device(np.clip(t, 0, K.MAX_D).astype(np.uint32), D2, ratio).max() == 0


def test_verdict_on_equal_distances_and_extreme_ratios(matcher):
    D = np.arange(ALL_D, dtype=np.uint32)
    for ratio in (0.5, 0.7, 0.75, 1.0):
        assert not matcher.l2_ratio_test_device(D, D, ratio).any()
    got = matcher.l2_ratio_test_device(D, D, 1.0000001)
    np.testing.assert_array_equal(got, K.verdict(D, D, 1.0000001).astype(np.uint8))
    rng = np.random.default_rng(3)
    D1 = rng.integers(0, ALL_D, ALL_D).astype(np.uint32)
    assert not matcher.l2_ratio_test_device(D1, D, 0.0).any()
    got = matcher.l2_ratio_test_device(D1, D, 1e30)
    np.testing.assert_array_equal(got, (D != 0).astype(np.uint8))
    assert len(matcher.l2_ratio_test_device(D[:0], D[:0], 0.7)) == 0


# ---- many pairs ---------------------------------------------------------------------------------------------------------------

MANY_ROWS = (300, 0, 1, 40, 700, 33, 129, 257, 512, 5, 64, 2)


@pytest.fixture(scope="module")
def many():
    rng = np.random.default_rng(12)
    frames = [K.mixed(rng, n) for n in MANY_ROWS]
    pairs = [(a, b) for a in range(len(frames)) for b in range(len(frames))]      # self pairs included
    L.ro(*frames)
    return frames, pairs, {}


def test_all_ordered_pairs_of_12_matrices(matcher, chunk, many, pkg):
    frames, pairs, refs = many
    for ratio in (0.7, 1.0):
        got = check(matcher, chunk, frames, pairs, ratio, refs)
        again = matcher.score_pairs_ratio_l2(frames, pairs, ratio)         # the records are re-initialised every call
        np.testing.assert_array_equal(got, again)
        # other pair-mode work on the same handle in between, and the list call as a second witness
        rng = np.random.default_rng(7)
        ham = rng.integers(0, 256, (50, 32), dtype=np.uint8)
        matcher.match_pair(ham, ham[::-1].copy())
        matcher.knn2_pair_l2(frames[3], frames[0])
        _, offs = matcher.match_pairs_ratio_l2(frames, pairs, ratio)
        np.testing.assert_array_equal(got["good_count"], np.diff(np.asarray(offs, np.int64)))
        np.testing.assert_array_equal(matcher.score_pairs_ratio_l2(frames, pairs, ratio), got)
    self_pairs = [k for k, (a, b) in enumerate(pairs) if a == b and len(frames[a]) > 1]
    assert (got["min_dist_sq"][self_pairs] == 0).all() and len(self_pairs) == 10


def test_automatic_chunk(matcher, auto, many):
    """128-row chunks below 1024 items of 256 rows, 256-row chunks from there on."""
    frames, pairs, refs = many
    n1 = K.workgroups(frames, pairs, 256)
    assert n1 < AUTO_LARGE_ITEMS <= 12 * n1
    for rep, ch in ((1, 128), (12, 256)):
        assert auto_chunk(frames, pairs * rep) == ch
        check(matcher, ch, frames, pairs * rep, 0.75, refs)


N_MANY = 70_000


def test_70000_tiny_pairs_in_one_call(matcher, auto):
    rng = np.random.default_rng(41)
    z = np.zeros((1, 128), np.uint8)
    frames = [z, np.stack([l2ref.row_with_dsq(9), l2ref.row_with_dsq(4)]), K.mixed(rng, 3), np.concatenate([K.mixed(rng, 1), 255 - z])]
    combos = [(a, b) for a in range(4) for b in range(4)]
    pairs = np.array([combos[(k * 7) % 16] for k in range(N_MANY)], np.int32)
    want16 = {p: K.ref_score(frames[p[0]], frames[p[1]], 0.7) for p in combos}
    assert want16[(0, 1)] == (1, 4) and want16[(0, 0)] == (0, 0)       # (4, 9): 2 / 3 < 0.7; one train row: nothing counts
    got = matcher.score_pairs_ratio_l2(frames, pairs, 0.7)
    info = matcher.launch_info()
    assert info.pairs == N_MANY and info.workgroups == N_MANY
    want = np.array([want16[tuple(p)] for p in pairs.tolist()], np.int64)
    np.testing.assert_array_equal(got["good_count"], want[:, 0])
    np.testing.assert_array_equal(got["min_dist_sq"], want[:, 1])
    np.testing.assert_array_equal(matcher.score_pairs_ratio_l2(frames, pairs, 0.7), got)


# ---- tall ---------------------------------------------------------------------------------------------------------------------

TALL = {"train 0": lambda: L.tall_train(0), "trap": L.tall_trap, "query 33": lambda: L.tall_query(33)}


@pytest.mark.parametrize("name", tuple(TALL))
def test_tall(matcher, monkeypatch, name):
    """40 x 65535 (2048 train tiles behind one running list, the trap in the last one) and 65535 x 33 (512 / 256 items)."""
    c = TALL[name]()
    assert (len(c.query), len(c.train)) in ((40, L.MAX_ROWS), (L.MAX_ROWS, 33))
    ref = (c.ref, int(L.distances_sq(c.query, c.train).min()))
    for ch in (128, 256):
        monkeypatch.setenv("LCM_TUNE_L2_COUNT_CHUNK", str(ch))
        for ratio in (0.7, 1.0):
            got = score(matcher, ch, [c.query, c.train], [(0, 1)], ratio, name)[0]
            assert (int(got["good_count"]), int(got["min_dist_sq"])) == K.ref_score(c.query, c.train, ratio, ref), (name, ch, ratio)
    if name == "train 0":
        assert K.ref_score(c.query, c.train, 1.0, ref)[0] < len(c.query)      # the planted equal pairs fail at 1.0
    if name == "trap":
        assert K.ref_score(c.query, c.train, 0.7, ref) == (len(c.query), 0)


# ---- the loop search ------------------------------------------------------------------------------------------------------------

LOOP_K = 50


@pytest.fixture(scope="module")
def loop_case():
    frames = K.loop_frames(LOOP_K)
    refs = {}
    want, scored = K.loop_search_ref(frames, K.LOOP_GAP, K.LOOP_SKIP, 0.7, K.LOOP_MIN_ROWS, LOOP_K, refs)
    assert [w[:3] for w in want] == [(8, 4, LOOP_K + 5), (9, 1, LOOP_K)]
    return frames, refs, want, scored


def assert_candidates(got, want):
    assert [(int(c["current_frame_id"]), int(c["matched_frame_id"]), int(c["num_matches"])) for c in got] == [w[:3] for w in want]
    np.testing.assert_array_equal(got["similarity_score"].view(np.uint64), np.array([w[3] for w in want], np.float64).view(np.uint64))


def test_loop_search(matcher, chunk, loop_case, pkg):
    frames, refs, want, scored = loop_case
    args = dict(loop_gap=K.LOOP_GAP, skip=K.LOOP_SKIP, ratio=0.7, min_rows=K.LOOP_MIN_ROWS)
    got, n_pairs = matcher.loop_search_ratio_l2(frames, min_matches=LOOP_K, **args)
    assert n_pairs == scored and matcher.launch_info().pairs == scored        # skipped pairs are not scored at all
    adm = [i for i in range(len(frames)) if not K.LOOP_SKIP[i] and len(frames[i]) >= K.LOOP_MIN_ROWS]
    assert matcher.launch_info().workgroups == sum(K.items(len(frames[c]), chunk) for c in adm for p in adm if c - p >= K.LOOP_GAP)
    assert_candidates(got, want)
    # k - 1 survivors: a candidate only once the threshold comes down to it
    lower, _ = K.loop_search_ref(frames, K.LOOP_GAP, K.LOOP_SKIP, 0.7, K.LOOP_MIN_ROWS, LOOP_K - 1, refs)
    assert len(lower) == len(want) + 1 and lower[-1][:3] == (11, 6, LOOP_K - 1)
    got, _ = matcher.loop_search_ratio_l2(frames, min_matches=LOOP_K - 1, **args)
    assert_candidates(got, lower)
    # no skip flags, another gap
    for gap, skip in ((K.LOOP_GAP, None), (5, K.LOOP_SKIP), (11, None), (12, None)):
        w, s = K.loop_search_ref(frames, gap, skip, 0.7, K.LOOP_MIN_ROWS, LOOP_K, refs)
        got, n_pairs = matcher.loop_search_ratio_l2(frames, gap, skip=skip, ratio=0.7, min_rows=K.LOOP_MIN_ROWS, min_matches=LOOP_K)
        assert n_pairs == s
        assert_candidates(got, w)
    # cap one too small: refused, `out` untouched, the count reported
    out = np.zeros(len(lower) - 1, pkg.capi.CANDIDATE_DTYPE)
    out["num_matches"] = -7
    before = out.copy()
    n, npairs = C.c_size_t(0), C.c_size_t(0)
    fr, ptrs, rows = matcher._sift_frames(frames)
    sk = np.array(K.LOOP_SKIP, np.uint8)
    rp = pkg.capi.RatioLoopParams(0.7, K.LOOP_MIN_ROWS, LOOP_K - 1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda o, cap, p: matcher._lib.lcm_loop_search_ratio_l2(matcher._h, C.cast(ptrs, C.c_void_p), vp(rows), len(fr), vp(sk), K.LOOP_GAP,
                                                                  p, o, cap, C.byref(n), C.byref(npairs))
    assert call(vp(out), len(out), C.byref(rp)) == pkg.capi.ERR_CAPACITY
    assert n.value == len(lower) and out.tobytes() == before.tobytes()
    assert call(None, 0, C.byref(rp)) == pkg.capi.ERR_CAPACITY and n.value == len(lower)
    full = np.zeros(len(lower), pkg.capi.CANDIDATE_DTYPE)
    assert call(vp(full), len(full), C.byref(rp)) == 0 and n.value == len(lower) and npairs.value == scored
    assert_candidates(full, lower)


def test_loop_search_defaults(matcher, chunk):
    """rp = NULL: ratio 0.7, min_rows 100, min_matches 300."""
    rng = np.random.default_rng(77)
    frames = [rng.integers(0, 256, (n, 128), dtype=np.uint8) for n in (310, 99, 320, 100, 305, 301)]
    for i in range(300):
        frames[4][i] = L.near_copy(rng, frames[0][i], 1 + i % 4)      # (4, 0): 300 survivors
    for i in range(299):
        frames[5][i] = L.near_copy(rng, frames[2][i], 1 + i % 4)      # (5, 2): 299
    want, scored = K.loop_search_ref(frames, 2, None, 0.7, 100, 300)
    assert [w[:3] for w in want] == [(4, 0, 300)] and scored == 7       # frame 1 has 99 rows, frame 3 exactly 100
    got, n_pairs = matcher.loop_search_ratio_l2(frames, 2)
    assert n_pairs == scored
    assert_candidates(got, want)
    got, _ = matcher.loop_search_ratio_l2(frames, 2, min_matches=299)
    assert [(int(c["current_frame_id"]), int(c["matched_frame_id"]), int(c["num_matches"])) for c in got] == [(4, 0, 300), (5, 2, 299)]


# ---- errors -------------------------------------------------------------------------------------------------------------------

def test_errors(matcher, pkg, auto):
    m, E = matcher, pkg.capi
    rng = np.random.default_rng(5)
    q, t = K.mixed(rng, 20), K.mixed(rng, 30)

    def code(fn, *a, **kw):
        with pytest.raises(pkg.LcmError) as e:
            fn(*a, **kw)
        return e.value.code

    for bad in (float("nan"), -1.0):
        assert code(m.score_pairs_ratio_l2, [q, t], [(0, 1)], bad) == E.ERR_INVALID_ARG
        assert code(m.loop_search_ratio_l2, [q, t], 1, ratio=bad) == E.ERR_INVALID_ARG
        assert code(m.l2_ratio_test_device, [1], [2], bad) == E.ERR_INVALID_ARG
    for bad_pair in ((0, 2), (2, 0), (-1, 0), (0, -1)):
        assert code(m.score_pairs_ratio_l2, [q, t], [(0, 1), bad_pair], 0.7) == E.ERR_INVALID_ARG
    for gap in (0, -3):
        assert code(m.loop_search_ratio_l2, [q, t], gap) == E.ERR_INVALID_ARG
    assert code(m.loop_search_ratio_l2, [q, t], 1, min_rows=-1) == E.ERR_INVALID_ARG
    assert code(m.loop_search_ratio_l2, [q, t], 1, min_matches=-1) == E.ERR_INVALID_ARG
    assert code(m.l2_ratio_test_device, [K.MAX_D + 1], [5], 0.7) == E.ERR_INVALID_ARG
    assert code(m.l2_ratio_test_device, [5, 5], [5, K.MAX_D + 1], 0.7) == E.ERR_INVALID_ARG
    assert m.l2_ratio_test_device([K.MAX_D, 0], [K.MAX_D, 1], 1.5).tolist() == [1, 1]

    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = m._lib
    fr, ptrs, rows = m._sift_frames([q, t])
    P = C.cast(ptrs, C.c_void_p)
    pair = np.array([[0, 1]], np.int32)
    out = np.zeros(1, E.L2_SCORE_DTYPE)
    z = C.c_size_t(0)
    cands = np.zeros(4, E.CANDIDATE_DTYPE)
    assert lib.lcm_score_pairs_ratio_l2(m._h, P, vp(rows), 2, vp(pair), 1, 0.7, None) == E.ERR_INVALID_ARG
    assert lib.lcm_score_pairs_ratio_l2(m._h, P, vp(rows), 2, None, 1, 0.7, vp(out)) == E.ERR_INVALID_ARG
    assert lib.lcm_score_pairs_ratio_l2(m._h, None, vp(rows), 2, vp(pair), 1, 0.7, vp(out)) == E.ERR_INVALID_ARG
    assert lib.lcm_score_pairs_ratio_l2(m._h, P, None, 2, vp(pair), 1, 0.7, vp(out)) == E.ERR_INVALID_ARG
    assert lib.lcm_score_pairs_ratio_l2(m._h, P, vp(rows), 2, vp(pair), -1, 0.7, vp(out)) == E.ERR_INVALID_ARG
    assert lib.lcm_score_pairs_ratio_l2(m._h, P, vp(rows), -1, vp(pair), 1, 0.7, vp(out)) == E.ERR_INVALID_ARG
    null_frame = (C.c_void_p * 2)(None, t.ctypes.data)
    assert lib.lcm_score_pairs_ratio_l2(m._h, C.cast(null_frame, C.c_void_p), vp(rows), 2, vp(pair), 1, 0.7, vp(out)) == E.ERR_INVALID_ARG
    for bad_rows, want in ((np.array([-1, 30], np.int32), E.ERR_INVALID_ARG), (np.array([65536, 30], np.int32), E.ERR_CAPACITY)):
        assert lib.lcm_score_pairs_ratio_l2(m._h, P, vp(bad_rows), 2, vp(pair), 1, 0.7, vp(out)) == want
        assert lib.lcm_loop_search_ratio_l2(m._h, P, vp(bad_rows), 2, None, 1, None, vp(cands), 4, C.byref(z), None) == want
    assert lib.lcm_loop_search_ratio_l2(m._h, P, vp(rows), 2, None, 1, None, vp(cands), 4, None, None) == E.ERR_INVALID_ARG
    assert lib.lcm_loop_search_ratio_l2(m._h, None, vp(rows), 2, None, 1, None, vp(cands), 4, C.byref(z), None) == E.ERR_INVALID_ARG
    assert lib.lcm_loop_search_ratio_l2(m._h, P, vp(rows), 2, None, 1, None, vp(cands), 4, C.byref(z), None) == 0      # n_pairs_out optional
    d = np.array([3], np.uint32)
    ok = np.zeros(1, np.uint8)
    assert lib.lcm_l2_ratio_test_device(m._h, None, vp(d), 1, 0.7, vp(ok)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_ratio_test_device(m._h, vp(d), None, 1, 0.7, vp(ok)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_ratio_test_device(m._h, vp(d), vp(d), 1, 0.7, None) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_ratio_test_device(m._h, None, None, 0, 0.7, None) == 0
    with pytest.raises(ValueError):
        m.score_pairs_ratio_l2([q[:, :32], t], [(0, 1)], 0.7)
    m.set_params(cross_check=1)
    try:
        assert code(m.score_pairs_ratio_l2, [q, t], [(0, 1)], 0.7) == E.ERR_INVALID_ARG
        assert code(m.loop_search_ratio_l2, [q, t], 1) == E.ERR_INVALID_ARG
    finally:
        m.set_params(cross_check=0)
    check(m, 128, [q, t], [(0, 1), (1, 0), (0, 0)], 0.75)              # the handle still works

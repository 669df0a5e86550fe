"""The SIFT keyframe store (lcm_l2_db_*: lcm_l2_db.cpp, lcm_l2_store.hip) against tests/l2ref.py through tests/l2countcases.py
and, as a second witness, against the host-matrix calls on the same frames (lcm_score_pairs_ratio_l2,
lcm_match_pairs_ratio_l2, lcm_loop_search_ratio_l2).  Needs a real MI355X.

Every search runs with LCM_TUNE_L2_COUNT_CHUNK pinned to 128 and to 256 (k_l2_count_store<1> / <2>) and asserts the
workgroups that served it: sum over the scored pairs with two non-empty sides of ceil(query rows / chunk).  With
min_matches = 0 every scored pair is a candidate, so a search hands out the good_count of EVERY record it made."""
import ctypes as C

import numpy as np
import pytest

import l2cases as L
import l2countcases as K

pytestmark = pytest.mark.gpu

TILE = K.TILE


@pytest.fixture(params=(128, 256))
def chunk(request, monkeypatch):
    monkeypatch.setenv("LCM_TUNE_L2_COUNT_CHUNK", str(request.param))
    return request.param


@pytest.fixture
def store(matcher):
    """The session's matcher with an empty SIFT store, before and after."""
    matcher.l2_db_clear()
    yield matcher
    matcher.l2_db_clear()


@pytest.fixture
def fresh(pkg):
    """A matcher of its own: the store has never reserved anything (lcm_l2_db_clear keeps the arenas)."""
    m = pkg.Matcher()
    yield m
    m.close()


def fill(m, frames):
    for k, f in enumerate(frames):
        assert m.l2_db_append(f) == k
    assert m.l2_db_size() == len(frames)


def tiles(n):
    return -(-n // TILE)


def search_pairs(frames, gap, skip=None, min_rows=0, currs=None):
    """The (curr, past) pairs of src/main.cpp:1375-1388 in its order; currs: the outer loop's values (default: all)."""
    n = len(frames)
    skip = [0] * n if skip is None else skip
    adm = lambda f: not skip[f] and len(frames[f]) >= min_rows
    return [(c, p) for c in (range(gap, n) if currs is None else currs) if adm(c) for p in range(0, c - gap + 1) if adm(p)]


def triples(cands):
    return [(int(c["current_frame_id"]), int(c["matched_frame_id"]), int(c["num_matches"])) for c in cands]


def assert_candidates(got, want):
    assert triples(got) == [w[:3] for w in want]
    np.testing.assert_array_equal(got["similarity_score"].view(np.uint64), np.array([w[3] for w in want], np.float64).view(np.uint64))


def assert_launch(m, ch, frames, pairs, msg=""):
    live = [(a, b) for a, b in pairs if len(frames[a]) and len(frames[b])]
    if live:
        info = m.launch_info()
        assert info.workgroups == K.workgroups(frames, pairs, ch), (msg, ch, info.workgroups)
        assert info.route == 0 and info.pairs == len(live), msg
        assert info.distances == sum(len(frames[a]) * len(frames[b]) for a, b in live), msg
        assert info.kernel_ms > 0


def all_records(m, ch, frames, gap, skip=None, min_rows=1, ratio=0.7):
    """lcm_l2_db_loop_search with min_matches = 0: {(curr, past): good_count} of every scored pair, launch checked."""
    pairs = search_pairs(frames, gap, skip, min_rows)
    got, n_pairs = m.l2_db_loop_search(gap, skip=skip, ratio=ratio, min_rows=min_rows, min_matches=0, cap=max(len(pairs), 1))
    assert n_pairs == len(pairs) and [t[:2] for t in triples(got)] == pairs
    assert_launch(m, ch, frames, pairs)
    return got


# ---- round trip -------------------------------------------------------------------------------------------------------------

ROUND_ROWS = (0, 1, 31, 32, 33, 300, 700)


def test_round_trip_growth_truncate(fresh):
    m = fresh
    rng = np.random.default_rng(1)
    frames = [rng.integers(0, 256, (n, 128), dtype=np.uint8) for n in ROUND_ROWS]
    assert m.l2_db_size() == 0 and m.l2_db_info().frames == 0 and m.l2_db_info().tiles_used == 0 and m.l2_db_info().tiles_reserved == 0
    reserved, growths = m.l2_db_info().tiles_reserved, 0
    for k, f in enumerate(frames):
        assert m.l2_db_append(f) == k
        info = m.l2_db_info()
        assert info.frames == k + 1 == m.l2_db_size()
        assert info.tiles_used == sum(tiles(len(g)) for g in frames[: k + 1]) <= info.tiles_reserved
        if info.tiles_reserved != reserved:
            assert reserved == 0 or (info.tiles_reserved % reserved == 0 and info.tiles_reserved >= 2 * reserved)     # doubles
            growths += reserved != 0
            reserved = info.tiles_reserved
        assert info.device_bytes >= info.tiles_reserved * (2 * 4096 + 128)
    assert growths >= 3                                    # the arenas moved several times under the stored frames
    for k, f in enumerate(frames):
        assert m.l2_db_rows(k) == len(f)
        back = m.l2_db_read(k)
        assert back.shape == f.shape and back.tobytes() == f.tobytes(), k
    # truncate keeps the leading slots bit for bit and frees the tiles behind them; an append reuses them
    m.l2_db_truncate(5)
    assert m.l2_db_size() == 5 and m.l2_db_info().tiles_used == sum(tiles(n) for n in ROUND_ROWS[:5])
    assert m.l2_db_info().tiles_reserved == reserved
    assert m.l2_db_append(frames[6]) == 5
    for k, f in ((4, frames[4]), (5, frames[6])):
        assert m.l2_db_read(k).tobytes() == f.tobytes()
    m.l2_db_clear()
    assert m.l2_db_size() == 0 and m.l2_db_info().tiles_used == 0 and m.l2_db_info().tiles_reserved == reserved


# ---- explicit pairs -----------------------------------------------------------------------------------------------------------

MANY_ROWS = (300, 0, 1, 40, 700, 33, 129, 257, 512, 5, 64, 2)
N_COLLISIONS = 10


@pytest.fixture(scope="module")
def many():
    rng = np.random.default_rng(12)
    frames = [K.mixed(rng, n) for n in MANY_ROWS]
    pairs = [(a, b) for a in range(len(frames)) for b in range(len(frames))]      # self pairs included
    L.ro(*frames)
    return frames, pairs, {}


def test_all_ordered_pairs_of_12_stored_matrices(store, chunk, many):
    m = store
    frames, pairs, refs = many
    fill(m, frames)
    for ratio in (0.7, 1.0):
        got = m.l2_db_score_pairs(pairs, ratio)
        assert_launch(m, chunk, frames, pairs)
        want = K.ref_scores(frames, pairs, ratio, refs)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, m.score_pairs_ratio_l2(frames, pairs, ratio))
        np.testing.assert_array_equal(m.l2_db_score_pairs(pairs, ratio), got)       # the records are re-initialised every call
    assert len(m.l2_db_score_pairs([], 0.7)) == 0


def test_match_lists_of_stored_pairs_byte_for_byte(store, many, pkg):
    """... and rows that the rescan redoes over the RAW rows of the arena (tests/l2cases.py's collision cases)."""
    m = store
    frames, pairs, _ = many
    cases = L.collision_cases()
    picked = [cases[k] for k in np.linspace(0, len(cases) - 1, N_COLLISIONS).astype(int)]
    assert any(c.collide for c in picked) and any(not c.collide for c in picked) and any(c.near is not None for c in picked)
    frames = list(frames)
    pairs = list(pairs)
    coll_pair = []
    for c in picked:
        frames += [c.query, c.train]
        coll_pair.append(len(pairs))
        pairs.append((len(frames) - 2, len(frames) - 1))
    fill(m, frames)
    for ratio in (0.7, 1e30):
        want_lists, want_offs = m.match_pairs_ratio_l2(frames, pairs, ratio)
        want_wg = m.launch_info().workgroups
        got_lists, got_offs = m.l2_db_match_pairs_ratio(pairs, ratio)
        assert m.launch_info().workgroups == want_wg and m.launch_info().pairs == sum(1 for a, b in pairs if len(frames[a]) and len(frames[b]))
        np.testing.assert_array_equal(got_offs, want_offs)
        assert len(got_lists) == len(want_lists) == len(pairs)
        for g, w in zip(got_lists, want_lists):
            assert g.tobytes() == w.tobytes()
    for c, p in zip(picked, coll_pair):                      # ratio 1e30: every row's best neighbour, in (sqrtf(D), index) order
        assert (got_lists[p]["train_idx"] == c.want[0]).all() and len(got_lists[p]) == len(c.query), (c.D, c.collide)
    # capacity: one record too few is refused before anything is written
    total = int(want_offs[-1])
    with pytest.raises(pkg.LcmError) as e:
        m.l2_db_match_pairs_ratio(pairs, 1e30, cap=total - 1)
    assert e.value.code == pkg.capi.ERR_CAPACITY


# ---- the loop search ------------------------------------------------------------------------------------------------------------

LOOP_K = 50


@pytest.fixture(scope="module")
def loop_case():
    frames = K.loop_frames(LOOP_K)
    refs = {}
    want, scored = K.loop_search_ref(frames, K.LOOP_GAP, K.LOOP_SKIP, 0.7, K.LOOP_MIN_ROWS, LOOP_K, refs)
    assert [w[:3] for w in want] == [(8, 4, LOOP_K + 5), (9, 1, LOOP_K)]
    lower, _ = K.loop_search_ref(frames, K.LOOP_GAP, K.LOOP_SKIP, 0.7, K.LOOP_MIN_ROWS, LOOP_K - 1, refs)
    assert len(lower) == len(want) + 1 and lower[-1][:3] == (11, 6, LOOP_K - 1)
    return frames, refs, want, lower, scored


def test_loop_search(store, chunk, loop_case, pkg):
    m = store
    frames, refs, want, lower, scored = loop_case
    fill(m, frames)
    args = dict(skip=K.LOOP_SKIP, ratio=0.7, min_rows=K.LOOP_MIN_ROWS)
    got, n_pairs = m.l2_db_loop_search(K.LOOP_GAP, min_matches=LOOP_K, **args)
    assert n_pairs == scored
    assert_launch(m, chunk, frames, search_pairs(frames, K.LOOP_GAP, K.LOOP_SKIP, K.LOOP_MIN_ROWS))
    assert m.l2_db_info().table_bytes <= 32 * len(frames) + 8 * len(frames)
    assert_candidates(got, want)
    host, host_pairs = m.loop_search_ratio_l2(frames, K.LOOP_GAP, min_matches=LOOP_K, **args)
    assert host.tobytes() == got.tobytes() and host_pairs == n_pairs
    got, _ = m.l2_db_loop_search(K.LOOP_GAP, min_matches=LOOP_K - 1, **args)       # k - 1 survivors: one threshold lower
    assert_candidates(got, lower)
    for gap, skip in ((K.LOOP_GAP, None), (5, K.LOOP_SKIP), (11, None), (12, None)):
        w, s = K.loop_search_ref(frames, gap, skip, 0.7, K.LOOP_MIN_ROWS, LOOP_K, refs)
        got, n_pairs = m.l2_db_loop_search(gap, skip=skip, ratio=0.7, min_rows=K.LOOP_MIN_ROWS, min_matches=LOOP_K)
        assert n_pairs == s
        assert_candidates(got, w)
    # cap one too small: refused, `out` untouched, the count reported
    out = np.zeros(len(lower) - 1, pkg.capi.CANDIDATE_DTYPE)
    out["num_matches"] = -7
    before = out.copy()
    n, npairs = C.c_size_t(0), C.c_size_t(0)
    sk = np.array(K.LOOP_SKIP, np.uint8)
    rp = pkg.capi.RatioLoopParams(0.7, K.LOOP_MIN_ROWS, LOOP_K - 1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda o, cap: m._lib.lcm_l2_db_loop_search(m._h, vp(sk), K.LOOP_GAP, C.byref(rp), o, cap, C.byref(n), C.byref(npairs))
    assert call(vp(out), len(out)) == pkg.capi.ERR_CAPACITY
    assert n.value == len(lower) and out.tobytes() == before.tobytes()
    assert call(None, 0) == pkg.capi.ERR_CAPACITY and n.value == len(lower)
    full = np.zeros(len(lower), pkg.capi.CANDIDATE_DTYPE)
    assert call(vp(full), len(full)) == 0 and n.value == len(lower) and npairs.value == scored
    assert_candidates(full, lower)


def test_loop_search_defaults(store, chunk):
    """rp = NULL: ratio 0.7, min_rows 100, min_matches 300, as lcm_loop_search_ratio_l2."""
    m = store
    rng = np.random.default_rng(77)
    frames = [rng.integers(0, 256, (n, 128), dtype=np.uint8) for n in (310, 99, 320, 100, 305, 301)]
    for i in range(300):
        frames[4][i] = L.near_copy(rng, frames[0][i], 1 + i % 4)      # (4, 0): 300 survivors
    for i in range(299):
        frames[5][i] = L.near_copy(rng, frames[2][i], 1 + i % 4)      # (5, 2): 299
    want, scored = K.loop_search_ref(frames, 2, None, 0.7, 100, 300)
    assert [w[:3] for w in want] == [(4, 0, 300)] and scored == 7
    fill(m, frames)
    got, n_pairs = m.l2_db_loop_search(2)
    assert n_pairs == scored
    assert_candidates(got, want)
    assert_launch(m, chunk, frames, search_pairs(frames, 2, None, 100))
    host, _ = m.loop_search_ratio_l2(frames, 2)
    assert host.tobytes() == got.tobytes()
    got, _ = m.l2_db_detect_loops(4, 2)                             # ... and of the online call
    assert_candidates(got, want)
    got, _ = m.l2_db_loop_search(2, min_matches=299)
    assert triples(got) == [(4, 0, 300), (5, 2, 299)]


# ---- online equals bulk ---------------------------------------------------------------------------------------------------------

def test_online_walk_equals_bulk(store, chunk, loop_case):
    m = store
    frames, refs, want, lower, scored = loop_case
    args = dict(ratio=0.7, min_rows=K.LOOP_MIN_ROWS, min_matches=LOOP_K - 1)
    walked, walked_pairs = [], 0
    for curr, f in enumerate(frames):
        assert m.l2_db_size() == curr
        if not K.LOOP_SKIP[curr]:                                    # :1377 is the caller's
            got, n_pairs = m.l2_db_detect_loops(curr, K.LOOP_GAP, query=f, skip=K.LOOP_SKIP[:curr], **args)
            pairs = search_pairs(frames, K.LOOP_GAP, K.LOOP_SKIP, K.LOOP_MIN_ROWS, currs=[curr])
            assert n_pairs == len(pairs)
            if pairs:
                assert_launch(m, chunk, frames, pairs, f"curr {curr}")
            walked += triples(got)
            walked_pairs += n_pairs
            assert m.l2_db_size() == curr                            # the query is not stored
        assert m.l2_db_append(f) == curr
    bulk, bulk_pairs = m.l2_db_loop_search(K.LOOP_GAP, skip=K.LOOP_SKIP, **args)
    assert_candidates(bulk, lower)
    assert walked == triples(bulk) and walked_pairs == bulk_pairs == scored
    # every stored slot in place
    again, again_pairs = [], 0
    for curr in range(len(frames)):
        if K.LOOP_SKIP[curr]:
            continue
        got, n_pairs = m.l2_db_detect_loops(curr, K.LOOP_GAP, skip=K.LOOP_SKIP, **args)
        again += triples(got)
        again_pairs += n_pairs
    assert again == walked and again_pairs == scored
    # the caller's decision: a skipped `curr` is searched when asked for
    got, n_pairs = m.l2_db_detect_loops(10, K.LOOP_GAP, skip=K.LOOP_SKIP, ratio=0.7, min_rows=K.LOOP_MIN_ROWS, min_matches=0)
    assert K.LOOP_SKIP[10] and n_pairs == len([p for p in range(8) if not K.LOOP_SKIP[p] and K.LOOP_ROWS[p] >= K.LOOP_MIN_ROWS]) == len(got)


# ---- decode edges ---------------------------------------------------------------------------------------------------------------

EDGE_ROWS = (128, 300, 129, 0, 256, 257, 1, 300, 128, 33, 257, 129)


@pytest.fixture(scope="module")
def edge_case():
    rng = np.random.default_rng(31)
    frames = [K.mixed(rng, n) for n in EDGE_ROWS]
    L.ro(*frames)
    return frames, {}


@pytest.mark.parametrize("gap,skip,min_rows", (
    (1, None, 1),                                     # runs of 1, 2, ... pasts; chunks per run 1..3, partial last chunks
    (1, None, 0),                                     # the empty frame is admitted: its pairs are records without a launch
    (2, (1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), 1),     # curr 2 is admitted with NO admitted past: no run, no record; curr 4: a single past
    (11, None, 1),                                    # one run of one pair: the grid's first workgroup is its last run's
    (4, (0, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0), 30),
))
def test_decode_edges(store, chunk, edge_case, gap, skip, min_rows):
    m = store
    frames, refs = edge_case
    fill(m, frames)
    pairs = search_pairs(frames, gap, skip, min_rows)
    got = all_records(m, chunk, frames, gap, skip, min_rows)
    want = K.ref_scores(frames, pairs, 0.7, refs)
    np.testing.assert_array_equal(got["num_matches"], want["good_count"].astype(np.int32))
    host, _ = m.loop_search_ratio_l2(frames, gap, skip=skip, ratio=0.7, min_rows=min_rows, min_matches=0, cap=max(len(pairs), 1))
    assert host.tobytes() == got.tobytes()
    np.testing.assert_array_equal(m.l2_db_score_pairs(pairs, 0.7), want)
    counts = {}
    for c, _ in pairs:
        counts[c] = counts.get(c, 0) + 1
    if skip is not None and gap == 2:
        assert 2 not in counts and 3 not in counts and counts[4] == 1
    assert len(set(want["good_count"].tolist())) > 3 or len(pairs) < 4          # the records differ: a wrong decode shows


N_MANY, MANY_SAMPLE = 300, 500


@pytest.fixture(scope="module")
def many_runs():
    rng = np.random.default_rng(5)
    frames = [K.mixed(rng, int(n)) for n in rng.integers(33, 41, N_MANY)]
    pairs = search_pairs(frames, 1, None, 1)
    assert len(pairs) == 44_850
    sample = np.random.default_rng(6).choice(len(pairs), MANY_SAMPLE, replace=False)
    want = K.ref_scores(frames, [pairs[k] for k in sample], 0.7)
    assert len(set(want["good_count"].tolist())) > 5
    return frames, pairs, sample, want


def test_299_runs_from_tables_that_grow_with_the_frames(store, chunk, many_runs):
    m = store
    frames, pairs, sample, want = many_runs
    fill(m, frames)
    got, n_pairs = m.l2_db_loop_search(1, ratio=0.7, min_rows=1, min_matches=0, cap=len(pairs))
    info = m.launch_info()
    assert n_pairs == len(pairs) == len(got) == info.pairs == info.workgroups        # one chunk per pair at 33..40 rows
    assert m.l2_db_info().table_bytes <= 64 * (N_MANY + 1)
    assert [t[:2] for t in triples(got)] == pairs
    host = m.score_pairs_ratio_l2(frames, pairs, 0.7)
    np.testing.assert_array_equal(got["num_matches"], host["good_count"].astype(np.int32))
    np.testing.assert_array_equal(got["num_matches"][sample], want["good_count"].astype(np.int32))
    np.testing.assert_array_equal(host[sample], want)


# ---- stale tiles ----------------------------------------------------------------------------------------------------------------

def test_stale_pad_rows_of_a_reused_tile(store, chunk):
    """A truncated 64-row frame leaves rows in the tile that a 33-row frame's pad rows then occupy: rows that would be the
    best train row (pad_train_case: D below every planted one), or pass as query rows (pad_query_case: D1 = 0)."""
    m = store
    q, t = K.pad_train_case(33)
    old = np.repeat(q[:1], 64, axis=0)                               # as train rows: at D = 0 from query row 0
    assert K.ref_score(q, np.concatenate([t, old[:31]]), 0.7)[0] < len(q)
    m.l2_db_append(old)
    m.l2_db_truncate(0)
    fill(m, [t, q])
    for ratio in (0.7, 0.75, 1.0):
        want = K.ref_score(q, t, ratio)
        assert want == (len(q), 0)
        assert tuple(m.l2_db_score_pairs([(1, 0)], ratio)[0]) == want
        got, _ = m.l2_db_detect_loops(1, 1, ratio=ratio, min_rows=1, min_matches=0)
        assert triples(got) == [(1, 0, want[0])]
    m.l2_db_clear()
    q, t = K.pad_query_case(33)
    old = np.full((64, 128), 128, np.uint8)                          # as query rows: D1 = 0 from train row 3, they pass
    assert K.ref_score(np.concatenate([q, old[:31]]), t, 0.7) == (31, 0)
    fill(m, [t, old])
    m.l2_db_truncate(1)
    assert m.l2_db_append(q) == 1
    for ratio, count in ((0.7, 0), (1.0, 0), (1.5, len(q))):
        want = K.ref_score(q, t, ratio)
        assert want == (count, 2)
        assert tuple(m.l2_db_score_pairs([(1, 0)], ratio)[0]) == want
        got, _ = m.l2_db_loop_search(1, ratio=ratio, min_rows=1, min_matches=0)
        assert triples(got) == [(1, 0, count)]
        assert_launch(m, chunk, [t, q], [(1, 0)])


# ---- growth, interleaving, staging ----------------------------------------------------------------------------------------------

def test_growth_between_searches_and_other_calls_in_between(store, chunk, edge_case):
    m = store
    frames, refs = edge_case
    fill(m, frames)
    first = all_records(m, chunk, frames, 2)
    scores = m.l2_db_score_pairs(search_pairs(frames, 2, None, 1), 0.7)
    # Hamming calls and host-matrix L2 calls between two searches of the store
    rng = np.random.default_rng(7)
    ham = rng.integers(0, 256, (50, 32), dtype=np.uint8)
    m.match_pair(ham, ham[::-1].copy())
    m.knn2_pair_l2(frames[1], frames[4])
    m.score_pairs_ratio_l2(frames[:3], [(0, 1), (2, 1)], 0.75)
    m.match_pairs_ratio_l2(frames[:3], [(1, 2)], 0.7)
    assert all_records(m, chunk, frames, 2).tobytes() == first.tobytes()
    # appends until the arenas have moved; the old pairs' records are unchanged
    reserved = m.l2_db_info().tiles_reserved
    more = list(frames)
    while m.l2_db_info().tiles_reserved == reserved:
        more.append(K.mixed(rng, 200))
        m.l2_db_append(more[-1])
    assert len(more) > len(frames)
    for k, f in enumerate(frames):
        assert m.l2_db_read(k).tobytes() == f.tobytes()
    after = all_records(m, chunk, more, 2)
    old = after[after["current_frame_id"] < len(frames)]
    assert old.tobytes() == first.tobytes()
    np.testing.assert_array_equal(m.l2_db_score_pairs(search_pairs(frames, 2, None, 1), 0.7), scores)


def test_host_query_staged_in_the_free_tail(fresh, chunk):
    m = fresh
    rng = np.random.default_rng(9)
    frames = [K.mixed(rng, n) for n in (300, 129, 40)]
    query = K.mixed(rng, 700)
    fill(m, frames)
    info = m.l2_db_info()
    assert info.tiles_reserved - info.tiles_used < tiles(700)        # the free tail is too small: the arenas grow
    pairs = [(3, p) for p in range(3)]
    want = K.ref_scores(frames + [query], pairs, 0.7)
    assert len(set(want["good_count"].tolist())) == 3
    got, n_pairs = m.l2_db_detect_loops(3, 1, query=query, ratio=0.7, min_rows=1, min_matches=0)
    assert n_pairs == 3 and triples(got) == [(3, p, int(want["good_count"][p])) for p in range(3)]
    assert_launch(m, chunk, frames + [query], pairs)
    grown = m.l2_db_info()
    assert grown.tiles_reserved - info.tiles_used >= tiles(700) and grown.tiles_used == info.tiles_used and grown.frames == 3
    for k, f in enumerate(frames):
        assert m.l2_db_read(k).tobytes() == f.tobytes()
    # an append overwrites the stage; the same query again, now also against the new frame
    frames.append(K.mixed(rng, 257))
    assert m.l2_db_append(frames[3]) == 3
    pairs = [(4, p) for p in range(4)]
    want = K.ref_scores(frames + [query], pairs, 0.7)
    got, n_pairs = m.l2_db_detect_loops(4, 1, query=query, ratio=0.7, min_rows=1, min_matches=0)
    assert n_pairs == 4 and triples(got) == [(4, p, int(want["good_count"][p])) for p in range(4)]
    assert m.l2_db_read(3).tobytes() == frames[3].tobytes()
    # an empty host query and one below min_rows score nothing
    assert m.l2_db_detect_loops(4, 1, query=query[:0], ratio=0.7, min_rows=1, min_matches=0)[1] == 0
    assert m.l2_db_detect_loops(4, 1, query=query[:39], ratio=0.7, min_rows=40, min_matches=0)[1] == 0
    got, n_pairs = m.l2_db_detect_loops(4, 1, query=query[:0], ratio=0.7, min_rows=0, min_matches=0)
    assert n_pairs == 4 and [(t[1], t[2]) for t in triples(got)] == [(p, 0) for p in range(4)] and (got["similarity_score"] == 0.0).all()


# ---- limits and errors ----------------------------------------------------------------------------------------------------------

def test_65535_row_frame_on_either_side(store, monkeypatch):
    m = store
    c = L.tall_trap()
    small, tall = c.query, c.train
    assert (len(small), len(tall)) == (40, L.MAX_ROWS)
    fwd = (c.ref, int(L.distances_sq(small, tall).min()))
    back = (L.knn2(tall, small), int(L.distances_sq(tall, small).min()))
    fill(m, [tall, small])
    assert m.l2_db_rows(0) == L.MAX_ROWS and m.l2_db_read(0).tobytes() == tall.tobytes()
    for ch in (128, 256):
        monkeypatch.setenv("LCM_TUNE_L2_COUNT_CHUNK", str(ch))
        for ratio in (0.7, 1.5):
            want_f, want_b = K.ref_score(small, tall, ratio, fwd), K.ref_score(tall, small, ratio, back)
            got = m.l2_db_score_pairs([(1, 0), (0, 1)], ratio)
            assert_launch(m, ch, [tall, small], [(1, 0), (0, 1)])
            assert [tuple(int(v) for v in r) for r in got] == [want_f, want_b], (ch, ratio)
            cand, _ = m.l2_db_detect_loops(1, 1, ratio=ratio, min_rows=1, min_matches=0)             # 40 x 65535, in place
            assert triples(cand) == [(1, 0, want_f[0])]
            assert_launch(m, ch, [tall, small], [(1, 0)])
            cand, _ = m.l2_db_detect_loops(2, 1, query=tall, skip=[1, 0], ratio=ratio, min_rows=1, min_matches=0)   # 65535 x 40, staged
            assert triples(cand) == [(2, 1, want_b[0])]
            assert m.launch_info().workgroups == K.items(L.MAX_ROWS, ch)
    assert K.ref_score(small, tall, 0.7, fwd) == (40, 0) and K.ref_score(tall, small, 1.5, back)[0] > 0
    # 65536 rows: refused before a byte is read
    buf = np.zeros((1, 128), np.uint8)
    n, z = C.c_int32(-5), C.c_size_t(0)
    vp = buf.ctypes.data_as(C.c_void_p)
    assert m._lib.lcm_l2_db_append(m._h, vp, 65536, C.byref(n)) == -4 and n.value == -5 and m.l2_db_size() == 2
    assert m._lib.lcm_l2_db_detect_loops(m._h, 2, vp, 65536, None, 1, None, None, 0, C.byref(z), None) == -4
    assert m._lib.lcm_l2_db_append(m._h, vp, -1, None) == -1


def test_errors(store, pkg):
    m, E = store, pkg.capi
    rng = np.random.default_rng(5)
    frames = [K.mixed(rng, 20), K.mixed(rng, 30), K.mixed(rng, 25)]
    fill(m, frames)

    def code(fn, *a, **kw):
        with pytest.raises(pkg.LcmError) as e:
            fn(*a, **kw)
        return e.value.code

    for gap in (0, -3):
        assert code(m.l2_db_loop_search, gap) == E.ERR_INVALID_ARG
        assert code(m.l2_db_detect_loops, 2, gap) == E.ERR_INVALID_ARG
    for bad in ((0, 3), (3, 0), (-1, 0), (0, -1)):
        assert code(m.l2_db_score_pairs, [(0, 1), bad], 0.7) == E.ERR_INVALID_ARG
        assert code(m.l2_db_match_pairs_ratio, [(0, 1), bad], 0.7, cap=100) == E.ERR_INVALID_ARG
    for slot in (3, -1):
        assert code(m.l2_db_rows, slot) == E.ERR_INVALID_ARG
        assert code(m.l2_db_detect_loops, slot, 1) == E.ERR_INVALID_ARG          # query == NULL: curr must be stored
    assert m._lib.lcm_l2_db_read(m._h, 3, None, 0) == E.ERR_INVALID_ARG
    assert m._lib.lcm_l2_db_read(m._h, 1, None, 29) == E.ERR_CAPACITY
    assert code(m.l2_db_truncate, 4) == E.ERR_INVALID_ARG and code(m.l2_db_truncate, -1) == E.ERR_INVALID_ARG
    for bad in (float("nan"), -1.0):
        assert code(m.l2_db_score_pairs, [(0, 1)], bad) == E.ERR_INVALID_ARG
        assert code(m.l2_db_match_pairs_ratio, [(0, 1)], bad) == E.ERR_INVALID_ARG
        assert code(m.l2_db_loop_search, 1, ratio=bad) == E.ERR_INVALID_ARG
        assert code(m.l2_db_detect_loops, 2, 1, ratio=bad) == E.ERR_INVALID_ARG
    assert code(m.l2_db_loop_search, 1, min_rows=-1) == E.ERR_INVALID_ARG
    assert code(m.l2_db_detect_loops, 2, 1, min_matches=-1) == E.ERR_INVALID_ARG
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    z = C.c_size_t(9)
    pair = np.array([[0, 1]], np.int32)
    out = np.zeros(1, E.L2_SCORE_DTYPE)
    cands = np.zeros(8, E.CANDIDATE_DTYPE)
    lib = m._lib
    assert lib.lcm_l2_db_score_pairs(m._h, vp(pair), 1, 0.7, None) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_score_pairs(m._h, None, 1, 0.7, vp(out)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_score_pairs(m._h, vp(pair), -1, 0.7, vp(out)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_match_pairs_ratio(m._h, vp(pair), 1, 0.7, vp(cands), 8, None) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_loop_search(m._h, None, 1, None, vp(cands), 8, None, None) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_detect_loops(m._h, 2, None, 0, None, 1, None, vp(cands), 8, None, None) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_loop_search(m._h, None, 1, None, vp(cands), 8, C.byref(z), None) == 0 and z.value == 0      # n_pairs_out optional
    assert lib.lcm_l2_db_info_read(m._h, None) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_rows(m._h, 0, None) == E.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        m.l2_db_append(frames[0][:, :32])
    m.set_params(cross_check=1)
    try:
        assert code(m.l2_db_score_pairs, [(0, 1)], 0.7) == E.ERR_INVALID_ARG
        assert code(m.l2_db_match_pairs_ratio, [(0, 1)], 0.7) == E.ERR_INVALID_ARG
        assert code(m.l2_db_loop_search, 1) == E.ERR_INVALID_ARG
        assert code(m.l2_db_detect_loops, 2, 1) == E.ERR_INVALID_ARG
        assert code(m.l2_db_detect_loops, 3, 1, query=frames[0]) == E.ERR_INVALID_ARG
    finally:
        m.set_params(cross_check=0)
    # the store still works, and nothing above changed it
    assert m.l2_db_size() == 3
    pairs = search_pairs(frames, 1, None, 1)
    np.testing.assert_array_equal(m.l2_db_score_pairs(pairs, 0.75), K.ref_scores(frames, pairs, 0.75))

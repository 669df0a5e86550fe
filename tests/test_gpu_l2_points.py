"""The store's loop correspondences made on the device (lcm_l2_db_append_kp, lcm_l2_db_read_kp, lcm_l2_db_match_points,
lcm_l2_db_detect_loops_points: lcm_l2_db.cpp, lcm_l2_emit.hip) against tests/l2ref.py (knn2 + ratio_filter) plus a numpy gather
of the keypoints and, as a second witness, against lcm_l2_db_match_pairs_ratio on the same store, whose `out` and `offsets`
they must equal byte for byte.  Needs a real MI355X.

Every list call runs with LCM_TUNE_L2_CHUNK pinned to 128 and to 256 (k_l2_score<1> / <2>).  A frame's keypoints are
distinct per slot and row, (slot << 16 | row) as float BITS in x: a gather from the wrong row, frame or tile shows, and every
comparison of points is on the bits."""
import ctypes as C

import numpy as np
import pytest

import l2cases as L
import l2countcases as K
import l2ref

pytestmark = pytest.mark.gpu

TILE = K.TILE


@pytest.fixture(params=(128, 256))
def chunk(request, monkeypatch):
    monkeypatch.setenv("LCM_TUNE_L2_CHUNK", str(request.param))
    return request.param


@pytest.fixture
def store(matcher):
    """The session's matcher with an empty SIFT store, before and after."""
    matcher.l2_db_clear()
    yield matcher
    matcher.l2_db_clear()


@pytest.fixture
def fresh(pkg):
    """A matcher of its own: the store has never reserved anything."""
    m = pkg.Matcher()
    yield m
    m.close()


def kp_for(slot, n):
    """float32[n, 2]: x = slot << 16 | row and y = x ^ 0xA5000000, as bits."""
    x = (np.uint32(slot) << np.uint32(16)) + np.arange(n, dtype=np.uint32)
    return np.stack([x, x ^ np.uint32(0xA5000000)], axis=1).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fill(m, frames, plain=(), kps=None):
    """Appends the frames, those at the positions `plain` without points; returns the keypoints per slot (None: none)."""
    out = []
    for k, f in enumerate(frames):
        if k in plain:
            assert m.l2_db_append(f) == k
            out.append(None)
        else:
            kp = kp_for(k, len(f)) if kps is None or kps[k] is None else kps[k]
            assert m.l2_db_append_kp(f, kp) == k
            out.append(kp)
    assert m.l2_db_size() == len(frames)
    return out


def ref_records(pkg, q, t, ratio, refs=None, key=None):
    """DMATCH_DTYPE[n] of one pair from l2ref: knn2 (over l2cases' exact distances) + ratio_filter, query order."""
    out = np.zeros(0, pkg.capi.DMATCH_DTYPE)
    if len(q) == 0 or len(t) == 0:
        return out
    if refs is not None and key in refs:
        ref = refs[key]
    else:
        ref = L.knn2(q, t)
        if refs is not None:
            refs[key] = ref
    rows, train, dist = l2ref.ratio_filter(ref[0], ref[1], ratio)
    out = np.zeros(len(rows), pkg.capi.DMATCH_DTYPE)
    out["query_idx"], out["train_idx"], out["distance"] = rows, train, dist
    return out


def ref_points(rec, kq, kt):
    return np.concatenate([bits(kq)[rec["query_idx"]], bits(kt)[rec["train_idx"]]], axis=1)


def check_lists(pkg, frames, kps, pairs, ratio, got, refs=None, sample=None, q_kp=None):
    """(out, pts, offsets) of a list call against the reference; sample: the pairs whose lists are compared (default: all).
    q_kp: the keypoints of a host query that stands for every pair's query side."""
    out, pts, offs = got
    ks = range(len(pairs)) if sample is None else sample
    for k in ks:
        a, b = pairs[k]
        want = ref_records(pkg, frames[a], frames[b], ratio, refs, (a, b))
        lo, hi = int(offs[k]), int(offs[k + 1])
        assert hi - lo == len(want), (k, a, b, hi - lo, len(want))
        assert out[lo:hi].tobytes() == want.tobytes(), (k, a, b)
        if pts is not None:
            np.testing.assert_array_equal(bits(pts[lo:hi]), ref_points(want, kps[a] if q_kp is None else q_kp, kps[b]), err_msg=str((k, a, b)))


def both_routes(pkg, m, frames, kps, pairs, ratio, refs=None, points=True):
    """lcm_l2_db_match_points == lcm_l2_db_match_pairs_ratio byte for byte == the reference; returns (out, pts, offsets)."""
    host_lists, host_offs = m.l2_db_match_pairs_ratio(pairs, ratio)
    host_info = m.launch_info()
    got = m.l2_db_match_points(pairs, ratio, points=points)
    out, pts, offs = got
    np.testing.assert_array_equal(offs, host_offs)
    assert out.tobytes() == b"".join(l.tobytes() for l in host_lists)
    assert (out["img_idx"] == 0).all()
    live = [(a, b) for a, b in pairs if len(frames[a]) and len(frames[b])]
    if live:
        info = m.launch_info()
        assert info.workgroups == host_info.workgroups and info.pairs == len(live) == host_info.pairs and info.route == 0
        assert info.kernel_ms > 0 and info.aux_kernel_ms > 0
        assert info.launches == host_info.launches + 3 + (1 if len(out) else 0)      # count, scan, offsets (+ emit): one slice each
    check_lists(pkg, frames, kps, pairs, ratio, got, refs)
    return got


# ---- shapes: every (query, train) size in ONE store and ONE call ------------------------------------------------------------------

Q_ROWS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513, 300)
T_ROWS = (1, 2, 33, 513)
SPECIAL = 9                                   # the 257-row query frame carries NaN, -0.0 and denormal coordinates


@pytest.fixture(scope="module")
def shapes():
    rng = np.random.default_rng(1)
    frames = [rng.integers(0, 256, (n, 128), dtype=np.uint8) for n in Q_ROWS + T_ROWS + (0, 40)]
    nq, nt = len(Q_ROWS), len(T_ROWS)
    empty, plain = nq + nt, nq + nt + 1
    pairs = []
    for a in range(nq):
        for b in range(nq, nq + nt):
            pairs.append((a, b))
            if (a + b) % 5 == 0:
                pairs.append((a, empty) if a % 2 else (empty, b))      # empty-side pairs between live ones
    pairs += [(empty, empty), (nq + 3, nq + 3), (nq + 2, 10)]           # a self pair, a train frame as query
    special = kp_for(SPECIAL, Q_ROWS[SPECIAL]).view(np.uint32).copy()
    special[0::4, 0] = 0x7FC12345                                      # quiet NaN with a payload
    special[1::4, 1] = 0x80000000                                      # -0.0
    special[2::4, 0] = 0x7F800001                                      # signalling NaN
    special[3::4, 1] = 0xFFFFFFFF
    L.ro(*frames)
    return frames, pairs, empty, plain, special.view(np.float32), {}


def test_every_shape_in_one_store_and_one_call(store, chunk, shapes, pkg):
    m = store
    frames, pairs, empty, plain, special, refs = shapes
    kps = fill(m, frames, plain=(plain,), kps=[special if k == SPECIAL else None for k in range(len(frames))])
    for k, kp in enumerate(kps):                                       # read_kp round trips, NaN and -0.0 included
        if kp is not None:
            back = m.l2_db_read_kp(k)
            assert back.shape == kp.shape and bits(back).tobytes() == bits(kp).tobytes(), k
    with pytest.raises(pkg.LcmError) as e:
        m.l2_db_read_kp(plain)
    assert e.value.code == pkg.capi.ERR_INVALID_ARG
    # ratio 0.98 on uniform random bytes keeps part of every larger pair's rows: from l2ref alone
    for a, b in pairs:
        if a != b and len(frames[a]) >= 255 and len(frames[b]) >= 2:
            kept = len(ref_records(pkg, frames[a], frames[b], 0.98, refs, (a, b)))
            assert 0.10 * len(frames[a]) <= kept <= 0.90 * len(frames[a]), (a, b, kept)
    for ratio in (1e30, 0.0, 0.98):
        out, pts, offs = both_routes(pkg, m, frames, kps, pairs, ratio, refs)
        counts = np.diff(offs.astype(np.int64))
        for (a, b), n in zip(pairs, counts):
            if ratio == 1e30:
                assert n == (len(frames[a]) if len(frames[b]) >= 2 else 0), (a, b)      # one train row: no second neighbour
            if ratio == 0.0:
                assert n == 0
        assert ratio == 0.0 or len(out) > 0
    # without points the call takes no notice of the arena
    both_routes(pkg, m, frames, kps, pairs, 0.98, refs, points=False)
    # a frame stored without points: refused when points are wanted (whichever side it is on), accepted when they are not
    for bad in ((0, plain), (plain, len(Q_ROWS) + 2)):
        with pytest.raises(pkg.LcmError) as e:
            m.l2_db_match_points([(7, len(Q_ROWS) + 2), bad], 0.98)
        assert e.value.code == pkg.capi.ERR_INVALID_ARG
        both_routes(pkg, m, frames, kps, [(7, len(Q_ROWS) + 2), bad], 0.98, refs, points=False)
    # ... and an EMPTY frame needs none
    out, pts, offs = m.l2_db_match_points([(empty, 3), (3, empty)], 0.98)
    assert len(out) == 0 and len(pts) == 0 and offs.tolist() == [0, 0, 0]


# ---- survivors at chosen rows only, the verdict exactly on its boundary -----------------------------------------------------------

PATTERN_ROWS = ((0,), (256,), (63, 64), (255, 256))
PATTERN_NQ = 257


@pytest.fixture(scope="module")
def planted():
    """Query frames of 257 rows: the zero row (boundary_frames' query) at the pattern's rows, the fillers' own row (all 255:
    two equal neighbours at D = 0, which fails at every ratio <= 1) elsewhere.  Train frames: per ratio, boundary cases
    with a small D2 and with one above 2^22 (the rescan's rows), each in its passing (D1 = t(D2) - 1) and failing form."""
    frames_b, pairs_b, cases = K.boundary_frames()
    queries = []
    for rows in PATTERN_ROWS:
        q = np.full((PATTERN_NQ, 128), 255, np.uint8)
        q[list(rows)] = 0
        queries.append(q)
    picked = {}
    for ratio in K.BOUNDARY_RATIOS:
        mine = [k for k, c in enumerate(cases) if c.ratio == ratio]
        low = [k for k in mine if cases[k].D2 < 1000][:2]
        high = [k for k in mine if cases[k].D2 > (1 << 22) + 1][:2]
        assert len(low) == 2 and len(high) == 2 and {cases[k].passes for k in low} == {cases[k].passes for k in high} == {True, False}
        picked[ratio] = low + high
    frames = queries + [frames_b[1 + k] for r in K.BOUNDARY_RATIOS for k in picked[r]]
    L.ro(*frames)
    return frames, picked, cases


def test_survivors_only_at_planted_rows(store, chunk, planted, pkg):
    m = store
    frames, picked, cases = planted
    kps = fill(m, frames)
    nqf = len(PATTERN_ROWS)
    at = nqf
    for ratio in K.BOUNDARY_RATIOS:
        trains = list(range(at, at + len(picked[ratio])))
        at += len(trains)
        pairs = [(a, b) for a in range(nqf) for b in trains]
        out, pts, offs = both_routes(pkg, m, frames, kps, pairs, ratio)
        for k, (a, b) in enumerate(pairs):
            case = cases[picked[ratio][b - trains[0]]]
            rows = out[int(offs[k]): int(offs[k + 1])]["query_idx"].tolist()
            assert rows == (list(PATTERN_ROWS[a]) if case.passes else []), (ratio, case, a)


# ---- the rescan dependency --------------------------------------------------------------------------------------------------------

N_COLLISIONS = 16


@pytest.fixture(scope="module")
def rescanned():
    cases = L.collision_cases()
    picked = [cases[k] for k in np.linspace(0, len(cases) - 1, N_COLLISIONS).astype(int)]
    assert any(c.collide for c in picked) and any(not c.collide for c in picked) and any(c.near is not None for c in picked)
    high = L.high_offsets()
    assert high.n_reordered > 100                                       # rows that only the rescan orders right
    frames, pairs = [], []
    for c in picked:
        frames += [c.query, c.train]
        pairs.append((len(frames) - 2, len(frames) - 1))
    frames += [high.query, high.train]
    pairs.append((len(frames) - 2, len(frames) - 1))
    return frames, pairs, picked, {}


def test_lists_read_the_rescanned_rows(store, chunk, rescanned, pkg):
    """Every row of these pairs is rewritten by k_l2_rescan: a list made from final_keys before it has the wrong train index
    (and point) on the colliding rows at ratio 1e30, and the wrong survivors at 1.0 (D1 = D < D2 = D + 1 but s1 == s2)."""
    m = store
    frames, pairs, picked, refs = rescanned
    kps = fill(m, frames)
    for ratio in (1e30, 1.0):
        out, pts, offs = both_routes(pkg, m, frames, kps, pairs, ratio, refs)
        if ratio == 1e30:
            for k, c in enumerate(picked):
                assert (out[int(offs[k]): int(offs[k + 1])]["train_idx"] == c.want[0]).all(), (c.D, c.collide)
    assert int(offs[-1] - offs[-2]) < len(frames[-2])                  # high_offsets at 1.0: the colliding rows fail


# ---- the store's life cycle -------------------------------------------------------------------------------------------------------

def tiles(n):
    return -(-n // TILE)


def test_points_arena_created_late_grows_truncates_and_clears(fresh, chunk, pkg):
    m = fresh
    rng = np.random.default_rng(3)
    frames = [K.mixed(rng, n) for n in (300, 33, 40)]
    kps = [None, None]
    assert m.l2_db_append(frames[0]) == 0 and m.l2_db_append(frames[1]) == 1
    before = m.l2_db_info()
    assert before.tiles_reserved - before.tiles_used >= tiles(40)
    assert before.device_bytes == before.tiles_reserved * (2 * 4096 + 128) + 64 * 8      # three arenas and the frame table
    # the first frame with points: the fourth arena, 256 bytes per tile of the store's capacity
    kps.append(kp_for(2, 40))
    assert m.l2_db_append_kp(frames[2], kps[2]) == 2
    after = m.l2_db_info()
    assert after.tiles_reserved == before.tiles_reserved and after.device_bytes == before.device_bytes + 256 * before.tiles_reserved
    # at least two growths under stored points
    growths, reserved = 0, after.tiles_reserved
    while growths < 2:
        frames.append(K.mixed(rng, int(rng.integers(100, 400))))
        kps.append(kp_for(len(frames) - 1, len(frames[-1])))
        assert m.l2_db_append_kp(frames[-1], kps[-1]) == len(frames) - 1
        if m.l2_db_info().tiles_reserved != reserved:
            growths, reserved = growths + 1, m.l2_db_info().tiles_reserved
    info = m.l2_db_info()
    assert info.device_bytes == info.tiles_reserved * (2 * 4096 + 128 + 256) + 64 * 8
    for k in range(2, len(frames)):
        assert bits(m.l2_db_read_kp(k)).tobytes() == bits(kps[k]).tobytes(), k
        assert m.l2_db_read(k).tobytes() == frames[k].tobytes()
    n = len(frames)
    pairs = [(a, b) for a in range(2, n) for b in range(2, n) if a != b]
    refs = {}
    both_routes(pkg, m, frames, kps, pairs, 0.7, refs)
    both_routes(pkg, m, frames, kps, pairs + [(0, 2), (2, 1)], 0.7, refs, points=False)      # the plain frames: lists only
    # truncate, then SHORTER frames into the reused tiles: their pad rows keep the old frames' points and raw rows
    m.l2_db_truncate(3)
    assert m.l2_db_size() == 3 and m.l2_db_info().tiles_reserved == reserved
    frames, kps = frames[:3], kps[:3]
    for rows, with_points in ((33, True), (70, False), (1, True), (65, True)):
        frames.append(K.mixed(rng, rows))
        if with_points:
            kps.append(kp_for(40 + len(frames), rows))                 # other bits than the slot's earlier tenant had
            assert m.l2_db_append_kp(frames[-1], kps[-1]) == len(frames) - 1
        else:
            kps.append(None)
            assert m.l2_db_append(frames[-1]) == len(frames) - 1
    with pytest.raises(pkg.LcmError) as e:
        m.l2_db_read_kp(4)                                             # stale points lie under it: not this frame's
    assert e.value.code == pkg.capi.ERR_INVALID_ARG
    pointed = [k for k in range(len(frames)) if kps[k] is not None]
    for k in pointed:
        assert bits(m.l2_db_read_kp(k)).tobytes() == bits(kps[k]).tobytes(), k
    both_routes(pkg, m, frames, kps, [(a, b) for a in pointed for b in pointed], 1e30)
    both_routes(pkg, m, frames, kps, [(a, b) for a in pointed for b in pointed], 0.7)
    m.l2_db_clear()
    assert m.l2_db_size() == 0 and m.l2_db_info().tiles_used == 0 and m.l2_db_info().tiles_reserved == reserved
    kps = fill(m, frames[3:5])
    both_routes(pkg, m, frames[3:5], kps, [(0, 1), (1, 0)], 1e30)


# ---- capacity ---------------------------------------------------------------------------------------------------------------------

def test_capacity_one_too_small(store, chunk, pkg):
    m, E = store, pkg.capi
    rng = np.random.default_rng(4)
    frames = [K.mixed(rng, n) for n in (70, 300, 33, 0)]
    kps = fill(m, frames)
    pairs = [(0, 1), (3, 1), (1, 2), (2, 0)]
    out, pts, offs = both_routes(pkg, m, frames, kps, pairs, 0.7)
    total = len(out)
    assert total > 10
    o = np.zeros(total, E.DMATCH_DTYPE)
    o["query_idx"] = -7
    p = np.full((total, 4), 3.5, np.float32)
    before_o, before_p = o.tobytes(), p.tobytes()
    for points in (True, False):
        with pytest.raises(pkg.LcmError) as e:
            m.l2_db_match_points(pairs, 0.7, cap=total - 1, points=points, out=o, pts=p if points else None)
        assert e.value.code == E.ERR_CAPACITY
        assert int(m.last_offsets[len(pairs)]) == total and o.tobytes() == before_o and p.tobytes() == before_p
        np.testing.assert_array_equal(m.last_offsets, offs)
    off = np.zeros(len(pairs) + 1, np.uintp)
    pr = np.array(pairs, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert m._lib.lcm_l2_db_match_points(m._h, vp(pr), len(pairs), 0.7, None, None, 0, vp(off)) == E.ERR_CAPACITY      # out == NULL: cap 0
    assert int(off[-1]) == total
    got = m.l2_db_match_points(pairs, 0.7, cap=total, out=o, pts=p)     # exactly enough
    assert got[0].tobytes() == out.tobytes() and bits(got[1]).tobytes() == bits(pts).tobytes()


# ---- one iteration of the reference's outer loop ----------------------------------------------------------------------------------

LOOP_K = 50


@pytest.fixture(scope="module")
def loop_case():
    frames = K.loop_frames(LOOP_K)
    refs = {}
    want, scored = K.loop_search_ref(frames, K.LOOP_GAP, K.LOOP_SKIP, 0.7, K.LOOP_MIN_ROWS, LOOP_K, refs)
    lower, _ = K.loop_search_ref(frames, K.LOOP_GAP, K.LOOP_SKIP, 0.7, K.LOOP_MIN_ROWS, LOOP_K - 1, refs)
    assert [w[:3] for w in want] == [(8, 4, LOOP_K + 5), (9, 1, LOOP_K)] and lower[-1][:3] == (11, 6, LOOP_K - 1)
    return frames, want, lower


def check_detect(pkg, m, frames, kps, curr, got, plain_cands, q_kp=None):
    """The candidates are lcm_l2_db_detect_loops's, the lists the reference's for (curr, matched)."""
    cands, n_pairs, out, pts, offs = got
    assert cands.tobytes() == plain_cands[0].tobytes() and n_pairs == plain_cands[1]
    pairs = [(curr, int(c["matched_frame_id"])) for c in cands]
    assert len(offs) == len(pairs) + 1 and int(offs[0]) == 0 and int(offs[-1]) == len(out)
    check_lists(pkg, frames, kps, pairs, 0.7, (out, pts, offs), q_kp=q_kp)
    assert [int(offs[k + 1] - offs[k]) for k in range(len(pairs))] == [int(c["num_matches"]) for c in cands]
    return pairs


def test_detect_loops_points(store, chunk, loop_case, pkg):
    m, E = store, pkg.capi
    frames, want, lower = loop_case
    args = dict(skip=K.LOOP_SKIP, ratio=0.7, min_rows=K.LOOP_MIN_ROWS)
    kps = fill(m, frames)
    seen = {}
    for min_matches, expect in ((LOOP_K, want), (LOOP_K - 1, lower)):
        found = []
        for curr in range(len(frames)):                                # query == NULL: the stored slot and its own points
            if K.LOOP_SKIP[curr]:
                continue
            plain = m.l2_db_detect_loops(curr, K.LOOP_GAP, min_matches=min_matches, **args)
            got = m.l2_db_detect_loops_points(curr, K.LOOP_GAP, min_matches=min_matches, **args)
            pairs = check_detect(pkg, m, frames, kps, curr, got, plain)
            found += pairs
            if pairs:                                                  # ... and the bulk form's second step on the same pairs
                o, p, f = m.l2_db_match_points(pairs, 0.7)
                assert o.tobytes() == got[2].tobytes() and bits(p).tobytes() == bits(got[3]).tobytes()
                np.testing.assert_array_equal(f, got[4])
                seen[curr] = got
            no_pts = m.l2_db_detect_loops_points(curr, K.LOOP_GAP, min_matches=min_matches, points=False, **args)
            assert no_pts[3] is None and no_pts[2].tobytes() == got[2].tobytes() and no_pts[0].tobytes() == got[0].tobytes()
        assert found == [w[:2] for w in expect]
    # capacities: the candidates first (the lists are not made), then the records
    cands = np.zeros(1, E.CANDIDATE_DTYPE)
    cands["num_matches"] = -7
    before = cands.tobytes()
    with pytest.raises(pkg.LcmError) as e:
        m.l2_db_detect_loops_points(9, K.LOOP_GAP, min_matches=0, cands=cands, cand_cap=1, cap=10000, **args)
    assert e.value.code == E.ERR_CAPACITY and m.last_n_cands.value > 1 and cands.tobytes() == before and int(m.last_offsets[0]) == 0
    total = len(seen[9][2])
    o = np.zeros(total, E.DMATCH_DTYPE)
    o["query_idx"] = -7
    p = np.full((total, 4), 3.5, np.float32)
    before_o, before_p = o.tobytes(), p.tobytes()
    with pytest.raises(pkg.LcmError) as e:
        m.l2_db_detect_loops_points(9, K.LOOP_GAP, min_matches=LOOP_K, cap=total - 1, out=o, pts=p, **args)
    assert e.value.code == E.ERR_CAPACITY and m.last_n_cands.value == 1 and int(m.last_offsets[1]) == total
    assert o.tobytes() == before_o and p.tobytes() == before_p
    got = m.l2_db_detect_loops_points(9, K.LOOP_GAP, min_matches=LOOP_K, cap=total, out=o, pts=p, **args)
    assert got[2].tobytes() == seen[9][2].tobytes() and bits(got[3]).tobytes() == bits(seen[9][3]).tobytes()


def test_detect_loops_points_host_query_walk(store, chunk, loop_case, pkg):
    """The online walk: every keyframe as a host query WITH its points before it is appended; other calls in between."""
    m = store
    frames, want, lower = loop_case
    args = dict(ratio=0.7, min_rows=K.LOOP_MIN_ROWS, min_matches=LOOP_K - 1)
    rng = np.random.default_rng(8)
    ham = rng.integers(0, 256, (50, 32), dtype=np.uint8)
    kps, found = [], []
    for curr, f in enumerate(frames):
        kp = kp_for(curr, len(f))
        if not K.LOOP_SKIP[curr]:
            plain = m.l2_db_detect_loops(curr, K.LOOP_GAP, query=f, skip=K.LOOP_SKIP[:curr], **args)
            got = m.l2_db_detect_loops_points(curr, K.LOOP_GAP, query=f, query_pts=kp, skip=K.LOOP_SKIP[:curr], **args)
            found += check_detect(pkg, m, frames, kps, curr, got, plain, q_kp=kp)
            assert m.l2_db_size() == curr                               # the query is not stored
            if curr == 9:
                # an append overwrites the stage; the query again, at the next position, then the store as it was
                assert m.l2_db_append_kp(frames[2], kp_for(curr, len(frames[2]))) == curr
                m.match_pair(ham, ham[::-1].copy())                     # a Hamming call and a host-matrix L2 call in between
                m.match_pairs_ratio_l2(frames[:3], [(1, 2)], 0.7)
                again = m.l2_db_detect_loops_points(curr + 1, K.LOOP_GAP + 1, query=f, query_pts=kp, skip=K.LOOP_SKIP[:curr] + (1,), **args)
                assert again[0]["matched_frame_id"].tolist() == got[0]["matched_frame_id"].tolist()
                assert again[2].tobytes() == got[2].tobytes() and bits(again[3]).tobytes() == bits(got[3]).tobytes()
                m.l2_db_truncate(curr)
                # points wanted but the query has none: refused; lists alone: served
                with pytest.raises(pkg.LcmError) as e:
                    m.l2_db_detect_loops_points(curr, K.LOOP_GAP, query=f, skip=K.LOOP_SKIP[:curr], **args)
                assert e.value.code == pkg.capi.ERR_INVALID_ARG
                bare = m.l2_db_detect_loops_points(curr, K.LOOP_GAP, query=f, skip=K.LOOP_SKIP[:curr], points=False, **args)
                assert bare[2].tobytes() == got[2].tobytes() and bare[3] is None
        assert m.l2_db_append_kp(f, kp) == curr
        kps.append(kp)
    assert found == [w[:2] for w in lower]


# ---- more pairs than gridDim.y holds ----------------------------------------------------------------------------------------------

N_MANY, MANY_SAMPLE = 70_000, 500


@pytest.fixture(scope="module")
def many_pairs(pkg):
    rng = np.random.default_rng(5)
    frames = [K.mixed(rng, int(n)) for n in rng.integers(33, 41, 9)] + [np.zeros((0, 128), np.uint8)]
    pr = rng.integers(0, 9, (N_MANY, 2))
    hit = rng.choice(N_MANY, 1500, replace=False)                        # empty-side pairs scattered among the live ones
    pr[hit, rng.integers(0, 2, len(hit))] = 9
    pairs = [(int(a), int(b)) for a, b in pr]
    refs = {}
    counts = {(a, b): len(ref_records(pkg, frames[a], frames[b], 0.7, refs, (a, b))) for a in range(len(frames)) for b in range(len(frames))}
    assert len(set(counts.values())) > 5 and sum(1 for a, b in pairs if a == 9 or b == 9) > 1000
    offs = np.concatenate([[0], np.cumsum([counts[p] for p in pairs])])
    sample = np.random.default_rng(6).choice(N_MANY, MANY_SAMPLE, replace=False)
    sample[:3] = (0, 65535, N_MANY - 1)                                  # both sides of the first slice's end, and the call's last pair
    return frames, pairs, refs, offs, sample


def test_70000_pairs_in_slices_of_the_grid_limit(store, chunk, many_pairs, pkg):
    m = store
    frames, pairs, refs, offs, sample = many_pairs
    kps = fill(m, frames)
    got = m.l2_db_match_points(pairs, 0.7, cap=int(offs[-1]))
    np.testing.assert_array_equal(got[2].astype(np.int64), offs)
    info = m.launch_info()
    live = sum(1 for a, b in pairs if a != 9 and b != 9)
    assert info.pairs == live == info.workgroups and live > 65535          # one item per pair at 33..40 rows; two slices
    assert info.launches == 3 + 2 + 2 + 2                                   # score, fold, rescan; count x 2, scan, offsets, emit x 2
    check_lists(pkg, frames, kps, pairs, 0.7, got, refs, sample=sample)


# ---- the error table --------------------------------------------------------------------------------------------------------------

def test_errors(store, pkg):
    m, E = store, pkg.capi
    rng = np.random.default_rng(5)
    frames = [K.mixed(rng, 20), K.mixed(rng, 30), K.mixed(rng, 25)]
    kps = fill(m, frames)

    def code(fn, *a, **kw):
        with pytest.raises(pkg.LcmError) as e:
            fn(*a, **kw)
        return e.value.code

    for bad in ((0, 3), (3, 0), (-1, 0), (0, -1)):
        assert code(m.l2_db_match_points, [(0, 1), bad], 0.7, cap=100) == E.ERR_INVALID_ARG
    for slot in (3, -1):
        assert code(m.l2_db_read_kp, slot) == E.ERR_INVALID_ARG
        assert code(m.l2_db_detect_loops_points, slot, 1) == E.ERR_INVALID_ARG      # query == NULL: curr must be stored
    for gap in (0, -3):
        assert code(m.l2_db_detect_loops_points, 2, gap) == E.ERR_INVALID_ARG
    for bad in (float("nan"), -1.0):
        assert code(m.l2_db_match_points, [(0, 1)], bad) == E.ERR_INVALID_ARG
        assert code(m.l2_db_detect_loops_points, 2, 1, ratio=bad) == E.ERR_INVALID_ARG
    assert code(m.l2_db_detect_loops_points, 2, 1, min_matches=-1) == E.ERR_INVALID_ARG
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = m._lib
    z, z2 = C.c_size_t(9), C.c_size_t(9)
    pair = np.array([[0, 1]], np.int32)
    out = np.zeros(64, E.DMATCH_DTYPE)
    pts = np.zeros((64, 4), np.float32)
    off = np.zeros(9, np.uintp)
    cands = np.zeros(8, E.CANDIDATE_DTYPE)
    buf = np.zeros((70, 128), np.uint8)
    fl = np.zeros((70, 2), np.float32)
    slot = C.c_int32(-5)
    assert lib.lcm_l2_db_read_kp(m._h, 1, None, 30) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_read_kp(m._h, 1, vp(fl), 29) == E.ERR_CAPACITY
    assert lib.lcm_l2_db_append_kp(m._h, None, vp(fl), 5, C.byref(slot)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_append_kp(m._h, vp(buf), None, 5, C.byref(slot)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_append_kp(m._h, vp(buf), vp(fl), -1, C.byref(slot)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_append_kp(m._h, vp(buf), vp(fl), 65536, C.byref(slot)) == E.ERR_CAPACITY
    assert slot.value == -5 and m.l2_db_size() == 3
    assert lib.lcm_l2_db_match_points(m._h, vp(pair), 1, 0.7, vp(out), vp(pts), 64, None) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_match_points(m._h, None, 1, 0.7, vp(out), vp(pts), 64, vp(off)) == E.ERR_INVALID_ARG
    assert lib.lcm_l2_db_match_points(m._h, vp(pair), -1, 0.7, vp(out), vp(pts), 64, vp(off)) == E.ERR_INVALID_ARG
    det = lambda n_c, offs, q=None, qp=None, nq=0: lib.lcm_l2_db_detect_loops_points(
        m._h, 2, q, qp, nq, None, 1, None, vp(cands), 8, n_c, C.byref(z2), vp(out), vp(pts), 64, offs)
    assert det(None, vp(off)) == E.ERR_INVALID_ARG
    assert det(C.byref(z), None) == E.ERR_INVALID_ARG
    assert det(C.byref(z), vp(off), vp(buf), vp(fl), 65536) == E.ERR_CAPACITY
    assert det(C.byref(z), vp(off), vp(buf), None, 20) == E.ERR_INVALID_ARG          # points wanted, the query has none
    assert det(C.byref(z), vp(off)) == 0 and z.value == 0                             # defaults: 25 rows are below min_rows = 100
    assert lib.lcm_l2_db_match_points(m._h, None, 0, 0.7, None, None, 0, vp(off)) == 0 and int(off[0]) == 0
    m.set_params(cross_check=1)
    try:
        assert code(m.l2_db_match_points, [(0, 1)], 0.7) == E.ERR_INVALID_ARG
        assert code(m.l2_db_detect_loops_points, 2, 1) == E.ERR_INVALID_ARG
        assert code(m.l2_db_detect_loops_points, 3, 1, query=frames[0], query_pts=kps[0]) == E.ERR_INVALID_ARG
    finally:
        m.set_params(cross_check=0)
    with pytest.raises(ValueError):
        m.l2_db_append_kp(frames[0], kps[1])                             # 20 rows, 30 points
    # the store still works, and nothing above changed it
    assert m.l2_db_size() == 3
    both_routes(pkg, m, frames, kps, [(0, 1), (2, 1), (1, 0)], 0.75)

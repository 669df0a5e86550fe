"""tests/l2storemodel.py without a device: what the random sequences of tests/test_gpu_l2_store_sequences.py reach (pinned per
seed, for exactly the seeds that file replays), the model against the scripted references the store's tests already use, and
every comparison of the GPU file fed one deliberately wrong answer."""
import numpy as np
import pytest

import epiref
import l2cases as L
import l2countcases as K
import l2ref
import l2storemodel as M
from verifychecks import check_closure

# What each stream gives (Coverage.summary()); a change of the generator shows here first.
PINNED = {
    4000: dict(fallbacks=19, growths_with_points=4, growths_staged=1, reused=57, plain_over_points=8, table_doubled=False),
    4001: dict(fallbacks=17, growths_with_points=4, growths_staged=1, reused=49, plain_over_points=8, table_doubled=False),
    4005: dict(fallbacks=13, growths_with_points=6, growths_staged=1, reused=51, plain_over_points=7, table_doubled=False),
    4006: dict(fallbacks=10, growths_with_points=4, growths_staged=2, reused=45, plain_over_points=6, table_doubled=False),
    4007: dict(fallbacks=18, growths_with_points=5, growths_staged=1, reused=42, plain_over_points=3, table_doubled=False),
    4009: dict(fallbacks=5, growths_with_points=5, growths_staged=1, reused=33, plain_over_points=5, table_doubled=True),
    4013: dict(fallbacks=6, growths_with_points=5, growths_staged=2, reused=21, plain_over_points=7, table_doubled=False),
    4017: dict(fallbacks=3, growths_with_points=4, growths_staged=1, reused=13, plain_over_points=4, table_doubled=False),
}
RUNS = [(s, M.STEPS, s == M.LIFT_SEED) for s in M.SEEDS] + [(s, M.TWIN_STEPS, False) for pair in M.TWIN_SEEDS for s in pair]


@pytest.fixture(scope="module")
def dry():
    return {seed: M.dry_run(seed, steps, lift) for seed, steps, lift in RUNS}


# ---- the dry run ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,steps,lift", RUNS)
def test_dry_run_reaches_what_the_sequences_are_for(dry, seed, steps, lift):
    cov = dry[seed]
    print(seed, cov.summary(), sorted(cov.edges), cov.kinds)
    assert cov.steps == steps
    cov.check(lift)           # every op kind, fallbacks <= 10 %, >= 2 growths under stored points, >= 1 by a staged query, >= 10 appends
    #                           into reused tiles, >= 1 plain append over old points, the table doubled in the lifted seed only
    assert cov.summary() == PINNED[seed]


def test_verification_edges_over_all_seeds(dry):
    reached = set().union(*(dry[s].edges for s in M.SEEDS))
    assert reached == {(k, e) for k in M.VERIFY_KINDS for e in M.EDGES}


def test_stream_depends_on_the_seed_alone():
    a, b = list(M.ops(4000, 60)), list(M.ops(4000, 60))
    assert [s.kind for s in a] == [s.kind for s in b] and [s.info for s in a] == [s.info for s in b]
    assert [M.describe(s) for s in a] == [M.describe(s) for s in b]
    assert [s.kind for s in a] != [s.kind for s in M.ops(4001, 60)]
    one = next(s for s in a if s.kind == "append_kp")
    again = next(s for s in b if s.kind == "append_kp")
    assert one.args["frame"].rows.tobytes() == again.args["frame"].rows.tobytes()


def test_frames_hold_what_the_issue_asks_for():
    """Family pairs with many shared rows, pairs with none, and a frame with NaN, -0.0 and all-ones keypoint bits per seed."""
    for seed in M.SEEDS[:2]:
        refs, shared, special = M.Refs(), [], 0
        for s in M.ops(seed, M.STEPS):
            if s.kind in ("append_kp", "append"):
                f = s.args["frame"]
                assert len(f) in M.ROW_CHOICES and len(s.frames) <= M.MAX_FRAMES
                if f.pts is not None and len(f):
                    b = M.bits(f.pts)
                    special += bool((b == 0x7FC12345).any() and (b == 0x80000000).any() and (b == 0xFFFFFFFF).any())
            if s.kind == "match_points":
                shared += [len(refs.records(q, t, 0.7)) for q, t in M.sides_of(s.frames, s.args["pairs"]) if q is not t]
        assert special >= 1 and min(shared) == 0 and any(0 < n < 8 for n in shared) and any(30 <= n <= 250 for n in shared), (special, sorted(shared))


# ---- the model against the scripted references ----------------------------------------------------------------------------------
def frames_of(mats):
    return [M.Frame(np.array(r), None, 10_000 + k) for k, r in enumerate(mats)]


def test_searches_equal_loop_search_ref():
    mats = K.loop_frames(50)
    frames, refs, krefs = frames_of(mats), M.Refs(), {}
    for gap, skip, min_matches in ((K.LOOP_GAP, K.LOOP_SKIP, 50), (K.LOOP_GAP, K.LOOP_SKIP, 49), (K.LOOP_GAP, None, 50), (5, K.LOOP_SKIP, 50),
                                   (11, None, 0), (12, None, 0)):
        want, scored = K.loop_search_ref(mats, gap, skip, 0.7, K.LOOP_MIN_ROWS, min_matches, krefs)
        got, n, sides = M.want_search(refs, frames, gap, skip, 0.7, K.LOOP_MIN_ROWS, min_matches)
        assert got == want and n == scored == len(sides)
        # one keyframe at a time, stored and as a host query before it is appended
        walked, walked_n = [], 0
        for curr in range(len(frames)):
            if skip is not None and skip[curr]:
                continue
            a = dict(curr=curr, gap=gap, skip=skip, ratio=0.7, min_rows=K.LOOP_MIN_ROWS, min_matches=min_matches)
            c, k, _, cand_sides = M.want_detect(refs, frames, a)
            h = dict(a, skip=None if skip is None else skip[:curr])
            assert M.want_detect(refs, frames[:curr], h, query=frames[curr])[:2] == (c, k)
            assert [len(refs.records(q, t, 0.7)) for q, t in cand_sides] == [x[2] for x in c]
            walked += c
            walked_n += k
        assert walked == want and walked_n == scored
    assert [w[:3] for w in K.loop_search_ref(mats, K.LOOP_GAP, K.LOOP_SKIP, 0.7, K.LOOP_MIN_ROWS, 50, krefs)[0]] == [(8, 4, 55), (9, 1, 50)]


def test_lists_equal_l2ref_on_the_collision_cases():
    cases = L.collision_cases()
    picked = [cases[k] for k in np.linspace(0, len(cases) - 1, 16).astype(int)]
    refs = M.Refs()
    for k, c in enumerate(picked):
        q, t = M.Frame(np.array(c.query), None, 2 * k), M.Frame(np.array(c.train), None, 2 * k + 1)
        idx, dist, _ = l2ref.knn2(c.query, c.train)
        for ratio in (0.7, 1.0, 1e30):
            rows, train, d = l2ref.ratio_filter(idx, dist, ratio)
            out, pts, offs = M.want_lists(refs, [(q, t)], ratio, False)
            assert pts is None and offs.tolist() == [0, len(rows)]
            assert (out["query_idx"].tolist(), out["train_idx"].tolist(), out["distance"].tobytes()) == (rows.tolist(), train.tolist(), d.tobytes())
            assert tuple(M.want_scores(refs, [(q, t)], ratio)[0]) == K.ref_score(c.query, c.train, ratio)
        assert (M.want_lists(refs, [(q, t)], 1e30, False)[0]["train_idx"] == c.want[0]).all()


ROUND_ROWS = (0, 1, 31, 32, 33, 300, 700)       # tests/test_gpu_l2_store.py::test_round_trip_growth_truncate


def test_reserved_tiles_of_the_round_trip():
    """That test asserts: tiles_used <= tiles_reserved, every change a doubling (a multiple, at least twice), at least three."""
    got = M.reserved_sequence(ROUND_ROWS)
    assert got == [1, 1, 2, 4, 8, 16, 64]
    used = np.cumsum([M.tiles(n) for n in ROUND_ROWS])
    assert (used <= got).all()
    changes = [(a, b) for a, b in zip(got, got[1:]) if a != b]
    assert len(changes) >= 3 and all(b % a == 0 and b >= 2 * a for a, b in changes)
    s = M.Store()
    for n in ROUND_ROWS:
        s.append(M.Frame(np.zeros((n, 128), np.uint8), None, 0))
    s.truncate(5)
    assert s.info() == dict(frames=5, tiles_used=5, tiles_reserved=64, device_bytes=64 * (2 * 4096 + 128) + 64 * 8)
    assert s.stage(700, True) is False and s.info()["device_bytes"] == 64 * (2 * 4096 + 128 + 256) + 64 * 8
    assert s.stage(32 * 60, False) is True and s.info()["tiles_reserved"] == 128 and s.info()["tiles_used"] == 5


def test_launch_arithmetic():
    f = lambda n: M.Frame(np.zeros((n, 128), np.uint8), None, 0)
    sides = [(f(300), f(600)), (f(0), f(5)), (f(129), f(1))]
    assert M.launch_of(sides, None, "count") == (2, 300 * 600 + 129, 3 + 2) == M.launch_of(sides, 128, "count")
    assert M.launch_of(sides, 256, "count") == (2, 300 * 600 + 129, 2 + 1)
    assert M.launch_of(sides, 128, "list") == (2, 300 * 600 + 129, 3 * 2 + 2) and M.launch_of(sides[1:2], None, "list") is None
    assert M.launch_of([(f(3), f(3))] * 1024, None, "count")[2] == 1024 and M.launch_of([(f(257), f(3))] * 512, None, "count")[2] == 1024


# ---- each check can fail ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def answers():
    """A right answer for every comparison, from one stream's stored frames."""
    s = max((x for x in M.ops(4000, M.STEPS) if x.kind == "match_points"), key=lambda x: len(x.frames))
    refs = M.Refs()
    pointed = [k for k, f in enumerate(s.frames) if f.pts is not None and len(f) > 8][:5]
    pairs = [(a, b) for a in pointed for b in pointed if a != b]
    sides = M.sides_of(s.frames, pairs)
    out, pts, offs = M.want_lists(refs, sides, 1e30, True)
    assert len(out) > 16 and (np.diff(offs) > 2).any()
    scores = M.want_scores(refs, sides, 0.7)
    cands, scored, _ = M.want_search(refs, s.frames, 1, None, 0.7, 0, 0)
    assert len(cands) >= 2
    got = np.zeros(len(cands), [("current_frame_id", "<i4"), ("matched_frame_id", "<i4"), ("num_matches", "<i4"), ("_pad", "<i4"),
                                ("similarity_score", "<f8")])
    for k, c in enumerate(cands):
        got[k] = (c[0], c[1], c[2], 0, c[3])
    return dict(lists=(out, pts.view(np.float32), offs), scores=scores, cands=(got, scored, cands))


def wrong(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def test_a_count_off_by_one_is_noticed(answers):
    scores = answers["scores"]
    M.check_scores(scores.copy(), scores)
    bad = scores.copy()
    bad["good_count"][len(bad) // 2] += 1
    wrong(M.check_scores, bad, scores)
    bad = scores.copy()
    bad["min_dist_sq"][0] ^= 1
    wrong(M.check_scores, bad, scores)
    out, pts, offs = answers["lists"]
    bad = offs.copy()
    bad[1] += 1
    wrong(M.check_lists, out, pts, bad, (out, pts.view(np.uint32), offs))
    info = dict(frames=3, tiles_used=7, tiles_reserved=16, device_bytes=100)
    M.check_info(dict(info), info)
    wrong(M.check_info, dict(info, device_bytes=99), info)


def test_two_swapped_records_and_a_neighbouring_point_are_noticed(answers):
    out, pts, offs = answers["lists"]
    want = (out, pts.view(np.uint32), offs)
    M.check_lists(out.copy(), pts.copy(), offs.copy(), want)
    bad = out.copy()
    bad[[3, 4]] = bad[[4, 3]]
    wrong(M.check_lists, bad, pts, offs, want)
    bad = pts.copy()
    bad[5] = pts[6]                                   # the point pair of the neighbouring record
    assert M.bits(bad[5]).tobytes() != M.bits(pts[5]).tobytes()
    wrong(M.check_lists, out, bad, offs, want)
    bad = pts.view(np.uint32).copy()
    bad[7, 3] ^= 0x80000000                           # a sign bit: -0.0 for 0.0 compares equal as floats, not as bits
    wrong(M.check_lists, out, bad.view(np.float32), offs, want)
    wrong(M.check_lists, out, None, offs, want)


def test_a_missing_candidate_is_noticed(answers):
    got, scored, cands = answers["cands"]
    M.check_candidates(got, scored, cands, scored)
    wrong(M.check_candidates, got[:-1], scored, cands, scored)
    wrong(M.check_candidates, np.delete(got, 0), scored, cands, scored)
    wrong(M.check_candidates, got, scored - 1, cands, scored)
    bad = got.copy()
    bad["similarity_score"][0] = np.nextafter(bad["similarity_score"][0], 2.0)
    wrong(M.check_candidates, bad, scored, cands, scored)


def test_a_flipped_mask_byte_and_best_iter_off_by_one_are_noticed():
    pts, _ = epiref.make_scene(60, 20, 4)
    offs = np.array([0, len(pts)], np.uintp)
    hyps = [epiref.hypotheses(pts, 0, 0, 64)]
    n_in, best, mask = epiref.closure(hyps[0][1], pts)
    res = np.zeros(1, [("E", "<f8", (9,)), ("n_points", "<i4"), ("n_inliers", "<i4"), ("best_iter", "<i4"), ("status", "<i4")])
    res[0] = (hyps[0][1][best], len(pts), n_in, best, 0)
    check_closure(res, mask, pts, offs, hyps, (0,))
    bad = mask.copy()
    bad[11] ^= 1
    wrong(check_closure, res, bad, pts, offs, hyps, (0,))
    bad = res.copy()
    bad["best_iter"] += 1
    wrong(check_closure, bad, mask, pts, offs, hyps, (0,))
    bad = res.copy()
    bad["n_inliers"] -= 1
    wrong(check_closure, bad, mask, pts, offs, hyps, (0,))


def test_edges_are_read_from_the_offsets():
    f = lambda n: M.Frame(np.zeros((n, 128), np.uint8), None, 0)
    sides = [(f(300), f(300)), (f(0), f(40)), (f(40), f(40))]
    assert M.edges_of(sides, [0, 257, 257, 264]) == {"blocks", "empty", "few"}
    assert M.edges_of(sides, [0, 256, 256, 264]) == {"empty"}
    assert M.edges_of(sides[:1], [0, 7]) == {"few"}

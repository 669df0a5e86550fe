"""tests/ratiomodel.py without a device: the streams the GPU file replays reach what they are there for (the figures DESIGN.md
lists), the model's searches equal ratioloopref's on the frame sets of the existing ratio tests, its lists equal knnref's insertion
loop, and every comparison function raises on one wrong answer."""
import numpy as np
import pytest

import knnref
import ratioloopref as R
import ratiomodel as M

# per seed: (fallbacks, rewinds, external sets with counts rewritten under their ids / one id under their counts, ticket steps, fused loop decisions with /
# without a candidate, distinct min_matches drawn, ratio entry points refused under cross_check) - DESIGN.md's table
FIGURES = {
    5107: (10, 2, 3, 3, 4, 27, 18, 9, 8),
    5113: (6, 6, 3, 4, 6, 25, 22, 15, 7),
    5117: (12, 5, 2, 3, 5, 30, 17, 11, 7),
    5126: (5, 8, 1, 4, 9, 27, 24, 18, 9),
    5140: (15, 3, 2, 7, 5, 28, 26, 13, 7),
    5145: (10, 7, 3, 4, 3, 28, 18, 23, 9),
}
# the interleaved pair, 120 steps each: the same figures, the op kinds the stream does not reach, the second-neighbour cases it meets
TWIN_FIGURES = {
    5150: ((12, 1, 2, 2, 3, 13, 13, 4, 7), [], ['d2_zero', 'no_second']),
    5162: ((6, 1, 1, 1, 3, 15, 10, 4, 5), [], ['d2_256', 'd2_zero', 'no_second']),
}
# per group seed: (fallbacks, searches that exchanged the shard arenas, searches that skipped the exchange, fused group searches
# with / without a candidate)
GROUP_FIGURES = {
    5204: (5, 25, 32, 12, 4),
    5205: (11, 27, 41, 14, 2),
    5207: (5, 24, 51, 14, 5),
}


@pytest.fixture(scope="module")
def refs():
    return M.Refs()


def figures(cov):
    return (cov.fallbacks, cov.rewinds, cov.ext_counts, cov.ext_ids, cov.with_tickets, cov.found, cov.not_found, len(cov.drawn), len(cov.refused))


@pytest.fixture(scope="module")
def runs(refs):
    return {seed: M.dry_run(seed, M.STEPS, refs) for seed in M.SEEDS}


@pytest.mark.parametrize("seed", M.SEEDS)
def test_streams_reach_what_they_are_for(runs, seed):
    cov = runs[seed]
    cov.check()
    assert figures(cov) == FIGURES[seed], (seed, figures(cov), cov.summary())


def test_every_entry_point_is_refused_under_cross_check(runs):
    refused = set().union(*(cov.refused for cov in runs.values()))
    assert refused == set(M.ENTRY_POINTS), sorted(set(M.ENTRY_POINTS) - refused)


@pytest.mark.parametrize("seed", [seed for seeds in M.TWIN_SEEDS for seed in seeds])
def test_twin_streams_reach_what_they_are_for(refs, seed):
    """The interleaved pair's streams are shorter: their figures and the op kinds each handle runs are pinned as they are."""
    cov = M.dry_run(seed, M.TWIN_STEPS, refs)
    assert cov.fallbacks * 10 <= cov.steps
    got = (figures(cov), sorted(set(M.KINDS) - set(cov.kinds)), sorted(cov.seen))
    assert got == TWIN_FIGURES[seed], got
    assert cov.fused_order == {("ratio", "classic"), ("classic", "ratio")}, cov.summary()


@pytest.mark.parametrize("world,seed", M.GROUP_RUNS)
def test_group_streams_reach_what_they_are_for(refs, world, seed):
    fig = M.group_dry_run(seed, M.GROUP_STEPS, world, refs)
    M.group_check(fig, M.GROUP_STEPS)
    assert (fig["fallbacks"], fig["gathered"], fig["skipped"], fig["found"], fig["none"]) == GROUP_FIGURES[seed], fig


def test_streams_depend_on_the_seed_alone():
    a = [(s.kind, M.describe(s)) for s in M.ops(M.SEEDS[0], 60)]
    b = [(s.kind, M.describe(s)) for s in M.ops(M.SEEDS[0], 60, M.Refs())]
    assert a == b


# ---- the model against the references the suite already trusts ------------------------------------------------------------------
def as_model(frames):
    return [fid for fid, _ in frames], [M.Frame(rows, ("set", k)) for k, (_, rows) in enumerate(frames)]


@pytest.mark.parametrize("name", ["boundary", "default", "group"])
def test_searches_equal_ratioloopref(name):
    frames, rps = {"boundary": (R.planted_frames(900, R.BOUNDARY_SPEC), [R.BOUNDARY_RP, (0.7, 41, 13), (1.0, 0, 0)]),
                   "default": (R.default_frames(), [None, R.DEFAULTS, (0.7, 100, 299)]),
                   "group": (R.planted_frames(903, R.GROUP_SPEC), [R.GROUP_RP, (0.7, 0, 1)])}[name]
    ref, refs = R.Ref(frames), M.Refs()
    ids, fr = as_model(frames)
    for gap in (1, 3):
        for rp in rps:
            ratio, min_rows, min_matches = R.DEFAULTS if rp is None else rp
            recs, offs, pairs = M.want_records(refs, ids, fr, gap, ratio)
            assert pairs == ref.pairs(gap) and offs[-1] == len(pairs)
            assert recs["good_count"].tolist() == [ref.count(c, s, ratio) for c, s in pairs]
            assert recs["n_train"].tolist() == [len(frames[s][1]) for _, s in pairs]
            want = ref.expected(gap, ratio, min_rows, min_matches)
            got = M.want_cands(recs, pairs, ids, fr, rp)
            assert [(int(c["current_frame_id"]), int(c["matched_frame_id"]), int(c["num_matches"])) for c in got] == [w[:3] for w in want]
            assert got["similarity_score"].view(np.uint64).tolist() == np.array([w[3] for w in want], np.float64).view(np.uint64).tolist()
            assert not got["_pad"].any()
            # one frame of the search
            c = len(ids) - 1
            one, _, one_pairs = M.want_records(refs, ids, fr, gap, ratio, [ids[c]], [fr[c]])
            got1 = M.want_cands(one, one_pairs, ids, fr, rp, [ids[c]], [fr[c]])
            assert [tuple(x)[:3] for x in got1] == [w[:3] for w in ref.expected(gap, ratio, min_rows, min_matches, only_query=c)]
    if name != "default":
        assert len(want) > 0


def test_lists_equal_the_insertion_loop():
    gen, refs = M.Frames(np.random.default_rng(77)), M.Refs()
    frames = [gen.make(n, ("crop", k)) for k, n in enumerate((0, 1, 2, 3, 9, 17, 24))]
    flags = set()
    for q in frames:
        for t in frames:
            if len(q) and len(t):
                idx, dist = knnref.insertion_knn2(q.rows, t.rows)
                M.check_knn2(refs.pair(q, t), (idx, dist))
                flags |= refs.flags[(q.uid, t.uid)]
            else:
                idx, dist = knnref.knn2(q.rows, t.rows)
            for ratio in M.RATIOS:
                rows, train, d = knnref.ratio_filter(idx, dist, ratio)
                got = refs.matches(q, t, ratio)
                assert (got["query_idx"].tolist(), got["train_idx"].tolist(), got["distance"].tolist()) == (rows.tolist(), train.tolist(), d.tolist())
                assert refs.record(q, t, ratio)[0] == len(rows) and refs.record(q, t, ratio)[2] == len(t)
    assert "no_second" in flags and "d2_zero" in flags


# ---- every comparison raises on one wrong answer --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample():
    """A small database's records, candidates and one list."""
    frames = R.planted_frames(905, [(40, 13), (41, 12), (3, 2), (64, 14), (40, 13)])
    ids, fr = as_model(frames)
    refs = M.Refs()
    recs, offs, pairs = M.want_records(refs, ids, fr, 1, 0.7)
    cands = M.want_cands(recs, pairs, ids, fr, (0.7, 3, 2))
    lists = M.want_lists(refs, [(fr[4], fr[0]), (fr[3], fr[1])], 0.7)
    assert len(cands) >= 3 and len(lists[0]) >= 4 and len(set(recs["n_train"][:3].tolist())) > 1
    return recs, offs, cands, lists, refs.pair(fr[4], fr[0])


def wrong(fn, got, want):
    fn(want, want)
    with pytest.raises(AssertionError):
        fn(got, want)


def test_comparisons_raise(sample):
    recs, offs, cands, (out, loffs), knn = sample
    bad = recs.copy(); bad["good_count"][2] += 1                              # a count off by one
    wrong(M.check_records, bad, recs)
    bad = recs.copy(); bad["n_train"][1] = recs["n_train"][2]                 # n_train of the neighbouring slot
    assert recs["n_train"][1] != recs["n_train"][2]
    wrong(M.check_records, bad, recs)
    bad = recs.copy(); bad["min_dist"][0] ^= 1
    wrong(M.check_records, bad, recs)
    wrong(M.check_records, recs[:-1], recs)
    bad = out.copy(); bad[[1, 2]] = bad[[2, 1]]                               # two list records swapped
    wrong(M.check_lists, (bad, loffs), (out, loffs))
    bad = loffs.copy(); bad[1] -= 1
    wrong(M.check_lists, (out, bad), (out, loffs))
    wrong(M.check_cands, np.delete(cands, 1), cands)                          # a candidate missing
    bad = cands.copy(); bad["similarity_score"].view(np.uint64)[0] += 1       # a similarity one ulp off
    wrong(M.check_cands, bad, cands)
    bad = cands.copy(); bad["_pad"][2] = 1                                    # a nonzero padding word
    wrong(M.check_cands, bad, cands)
    bad = cands.copy(); bad["matched_frame_id"][0] += 1
    wrong(M.check_cands, bad, cands)
    idx, dist = knn
    bad = idx.copy(); bad[0] = bad[0, ::-1]
    wrong(M.check_knn2, (bad, dist), knn)
    bad = dist.copy(); bad[3, 1] += 1
    wrong(M.check_knn2, (idx, bad), knn)
    wrong(M.check_equal, offs[:-1] + [offs[-1] + 1], offs)
    M.check_launch((10, 200, 7, 0), (10, 200, 7))
    M.check_launch(None, None)
    for got, want in ((None, (10, 200, 7)), ((10, 200, 7, 0), None)):         # a launch the model does not expect, and none where it does
        with pytest.raises(AssertionError):
            M.check_launch(got, want)
    for got in ((9, 200, 7, 0), (10, 201, 7, 0), (10, 200, 8, 0), (10, 200, 7, 1)):
        with pytest.raises(AssertionError):
            M.check_launch(got, (10, 200, 7))
    with pytest.raises(AssertionError):
        M.check_outputs([("records", recs), ("n", 3)], [("records", recs), ("n", 4)])
    with pytest.raises(AssertionError):
        M.check_outputs([("records", recs)], [("records", recs), ("n", 4)])

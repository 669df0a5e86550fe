"""The good-match filter `d <= max(ratio * min_d, dist_floor)` on every scoring route, at every (ratio, dist_floor) of
the grid, on planted frames (tests/planted.py) whose rows sit exactly at thr - 1, thr and thr + 1, in the far range
(min_d > 128, distances up to 256) and with first minima (and equal-distance decoys after them) on the kernels' seams.

The rule is written out separately in each route's epilogue / fold kernel: bulk plain (variants 0 / 1 and the argmin
checksum), train-lane (variants 2 / 3), packed (2- and 4-byte words, <= 2048 and > 2048 query rows), matrix-core
(variants 4 / 5), online split, cross_check, and the host-side match lists.  Every case compares with the oracle at the
same parameters (records and index checksums byte for byte, match lists and loop candidates field by field) and asserts
which route served the call.  With dist_floor >= 256 every query row is good, so the index checksum covers every row's
first-minimum index."""
import numpy as np
import pytest

import planted

pytestmark = pytest.mark.gpu

GRID = planted.GRID
# (kind, query rows, train rows[, option]): sizes around the 4-row padding, the 8-row groups, the 32-row tiles
SPECS = [("near", 33, 31), ("near", 5, 1), ("far", 3, 3), ("near", 4, 4), ("near", 64, 65), ("far", 31, 33, "tied"),
         ("near", 65, 63), ("far", 130, 130), ("near", 257, 257), ("near", 5, 5), ("far", 63, 64)]


def _restore(matcher, pkg):
    matcher.set_params(ratio=2, dist_floor=0, min_gap=30, min_matches=50, sim_threshold=0.15, cross_check=0)
    matcher.set_kernel_variant(0)
    matcher.set_tuning(pkg.capi.TUNE_PACKED, -1)
    matcher.set_tuning(pkg.capi.TUNE_ONLINE_SPLIT, -1)
    matcher.set_tuning(pkg.capi.TUNE_PAIR_HOST_FOLD, 1)
    matcher.clear()


def _fill(m, fr, n=None):
    m.clear()
    for f in range(fr.n_frames if n is None else n):
        m.append(int(fr.ids[f]), fr.frame(f))


def _self_pairs(ids, gap=1):
    pq, pt = [], []
    for c in range(len(ids)):
        for t in range(len(ids)):
            if ids[c] - ids[t] >= gap:
                pq.append(c); pt.append(t)
    return pq, pt


def _want_ext(oracle, fr, n_db, queries, q_ids, p):
    """Oracle records + index checksums of `query c against every stored frame i < n_db with q_ids[c] - ids[i] >= 1`."""
    stride = max(fr.rows.shape[1], max(len(q) for q in queries))
    rows = np.zeros((n_db + len(queries), stride, 32), np.uint8)
    rows[:n_db, : fr.rows.shape[1]] = fr.rows[:n_db]
    for c, q in enumerate(queries):
        rows[n_db + c, : len(q)] = q
    counts = np.concatenate([fr.counts[:n_db], [len(q) for q in queries]]).astype(np.int32)
    pq, pt, offs = [], [], [0]
    for c, qid in enumerate(q_ids):
        for i in range(n_db):
            if int(qid) - int(fr.ids[i]) >= 1:
                pq.append(n_db + c); pt.append(i)
        offs.append(len(pq))
    sc, sums = oracle.fast_score_pairs_idx(rows, counts, pq, pt, p, n_threads=8)
    return sc, sums, np.array(offs, np.int64)


def _bulk(matcher, pkg, n, route, argmin=True, **ext):
    """lcm_all_vs_all (and lcm_all_vs_all_argmin): (records, argmin records, checksums); both calls on `route`."""
    d, ds = matcher.dev_alloc(n * 8), matcher.dev_alloc(n * 4)
    try:
        got, got2, sums = np.zeros(n, pkg.capi.SCORE_DTYPE), np.zeros(n, pkg.capi.SCORE_DTYPE), np.zeros(n, np.uint32)
        matcher.all_vs_all(d, n, **ext)
        assert matcher.launch_info().route == route, "all_vs_all served by another route"
        matcher.sync(); matcher.dev_download(d, got)
        if argmin:
            matcher.all_vs_all_argmin(d, n, ds, **ext)
            assert matcher.launch_info().route == route, "all_vs_all_argmin served by another route"
            matcher.sync(); matcher.dev_download(d, got2); matcher.dev_download(ds, sums)
        return got, got2, sums
    finally:
        matcher.dev_free(d); matcher.dev_free(ds)


def _bulk_cases(pkg):
    R = pkg.capi
    # (variant, LCM_TUNE_PACKED, cross_check, route); variants 2 / 3 and cross_check with packing off
    return [(0, 0, 0, R.ROUTE_PLAIN), (1, 0, 0, R.ROUTE_PLAIN), (2, 0, 0, R.ROUTE_PLAIN), (3, 0, 0, R.ROUTE_PLAIN),
            (0, 1, 0, R.ROUTE_PACKED), (0, 2, 0, R.ROUTE_PACKED), (4, 0, 0, R.ROUTE_MATRIX), (5, 0, 0, R.ROUTE_MATRIX),
            (0, 0, 1, R.ROUTE_CROSS), (0, 0, 2, R.ROUTE_CROSS)]


@pytest.mark.parametrize("ratio,floor", GRID)
def test_bulk_self_search_every_route(matcher, oracle, pkg, ratio, floor):
    fr = planted.frames(SPECS, ratio, floor, seed=100)
    pq, pt = _self_pairs(fr.ids)
    try:
        _fill(matcher, fr)
        for variant, packed, cross, route in _bulk_cases(pkg):
            matcher.set_params(ratio=ratio, dist_floor=floor, min_gap=1, cross_check=cross)
            matcher.set_kernel_variant(variant)
            matcher.set_tuning(pkg.capi.TUNE_PACKED, packed)
            p = oracle.default_params(ratio=ratio, dist_floor=floor, min_gap=1, cross_check=cross)
            want, wsums = oracle.fast_score_pairs_idx(fr.rows, fr.counts, pq, pt, p, n_threads=8)
            n, _ = matcher.all_vs_all_plan()
            assert n == len(want)
            got, got2, sums = _bulk(matcher, pkg, n, route)
            tag = f"variant={variant} packed={packed} cross={cross}"
            np.testing.assert_array_equal(got, want, err_msg=tag)
            np.testing.assert_array_equal(got2, want, err_msg=tag + " (argmin kernel)")
            np.testing.assert_array_equal(sums, wsums, err_msg=tag + " (index checksums)")
        if floor >= 256:        # every row good: the checksum is the sum of EVERY query row's first-minimum index
            p = oracle.default_params(ratio=ratio, dist_floor=floor, min_gap=1)
            want, _ = oracle.fast_score_pairs_idx(fr.rows, fr.counts, pq, pt, p, n_threads=8)
            good = {(c, t): int(s["good_count"]) for c, t, s in zip(pq, pt, want)}
            assert all(good[(c, t)] == int(fr.counts[c]) for c, t, _ in fr.pairs)
    finally:
        _restore(matcher, pkg)


@pytest.mark.parametrize("ratio,floor", GRID)
def test_bulk_external_queries_and_fused_loops(matcher, oracle, pkg, ratio, floor):
    """The train frames stored, the query frames (ids interleaved with them) as an external query set; then the fused
    loop search over the self search with a loop test loose enough that the filter decides the candidate list."""
    fr = planted.frames(SPECS[:8], ratio, floor, seed=200, empty=False, duplicate=False)
    t_idx = [t for _, t, _ in fr.pairs]
    q_idx = [c for c, _, _ in fr.pairs]
    db = planted.Frames(fr.rows[t_idx], fr.counts[t_idx], fr.ids[t_idx], [])
    queries = [fr.frame(c) for c in q_idx]
    q_ids = fr.ids[q_idx]
    stride = max(len(q) for q in queries)
    q_rows = np.zeros((len(queries), stride, 32), np.uint8)
    for c, q in enumerate(queries):
        q_rows[c, : len(q)] = q
    q_counts = np.array([len(q) for q in queries], np.int32)
    R = pkg.capi
    d_rows, d_counts = matcher.dev_alloc(q_rows.nbytes), matcher.dev_alloc(q_counts.nbytes)
    try:
        _fill(matcher, db)
        matcher.dev_upload(d_rows, q_rows); matcher.dev_upload(d_counts, q_counts)
        ext = dict(d_query_rows=d_rows, d_query_counts=d_counts, q_ids=q_ids, q_stride_rows=stride)
        for variant, packed, cross, route in [(0, 0, 0, R.ROUTE_PLAIN), (0, 1, 0, R.ROUTE_PACKED),
                                              (4, 0, 0, R.ROUTE_MATRIX), (0, 0, 1, R.ROUTE_CROSS)]:
            matcher.set_params(ratio=ratio, dist_floor=floor, min_gap=1, cross_check=cross)
            matcher.set_kernel_variant(variant)
            matcher.set_tuning(R.TUNE_PACKED, packed)
            p = oracle.default_params(ratio=ratio, dist_floor=floor, min_gap=1, cross_check=cross)
            want, wsums, woffs = _want_ext(oracle, db, db.n_frames, queries, q_ids, p)
            n, offs = matcher.all_vs_all_plan(**ext)
            assert n == len(want) and np.array_equal(offs.astype(np.int64), woffs)
            got, got2, sums = _bulk(matcher, pkg, n, route, **ext)
            tag = f"variant={variant} packed={packed} cross={cross}"
            np.testing.assert_array_equal(got, want, err_msg=tag)
            np.testing.assert_array_equal(got2, want, err_msg=tag + " (argmin kernel)")
            np.testing.assert_array_equal(sums, wsums, err_msg=tag + " (index checksums)")
        # fused loop search on the whole planted database
        _fill(matcher, fr)
        pq, pt = _self_pairs(fr.ids)
        p = oracle.default_params(ratio=ratio, dist_floor=floor, min_gap=1, min_matches=2, sim_threshold=0.0)
        want, _ = oracle.fast_score_pairs_idx(fr.rows, fr.counts, pq, pt, p, n_threads=8)
        expect = []
        for s, c, t in zip(want, pq, pt):
            ok, sim = oracle.loop_test(int(s["good_count"]), int(fr.counts[c]), int(fr.counts[t]), p)
            if ok:
                expect.append((int(fr.ids[c]), int(fr.ids[t]), int(s["good_count"]), sim))
        assert 0 < len(expect) < len(pq)             # the loop test is decided pair by pair, not vacuous
        matcher.set_params(ratio=ratio, dist_floor=floor, min_gap=1, min_matches=2, sim_threshold=0.0, cross_check=0)
        matcher.set_kernel_variant(0)
        for packed, route in [(0, R.ROUTE_PLAIN), (1, R.ROUTE_PACKED)]:
            matcher.set_tuning(R.TUNE_PACKED, packed)
            cands, npairs = matcher.all_vs_all_loops(cap=len(pq))
            assert matcher.launch_info().route == route
            assert npairs == len(pq)
            got = [(int(c["current_frame_id"]), int(c["matched_frame_id"]), int(c["num_matches"]), float(c["similarity_score"]))
                   for c in cands]
            assert got == expect, f"packed={packed}"
    finally:
        matcher.dev_free(d_rows); matcher.dev_free(d_counts)
        _restore(matcher, pkg)


@pytest.mark.parametrize("ratio,floor", GRID)
def test_packed_query_frame_above_2048_rows(matcher, oracle, pkg, ratio, floor):
    """A 2500-row query frame (near and far planted, boundary rows at query rows 2047 / 2048) through the packed route
    in both word widths: 2-byte distances (lcm_all_vs_all) and 4-byte keys (argmin) — the nq > 2048 branches of both
    fold kernels."""
    fr = planted.frames([("near", 2500, 300), ("far", 2500, 70)], ratio, floor, seed=300, empty=False, duplicate=False)
    pq, pt = _self_pairs(fr.ids)
    try:
        _fill(matcher, fr)
        matcher.set_params(ratio=ratio, dist_floor=floor, min_gap=1)
        matcher.set_tuning(pkg.capi.TUNE_PACKED, 1)
        p = oracle.default_params(ratio=ratio, dist_floor=floor, min_gap=1)
        want, wsums = oracle.fast_score_pairs_idx(fr.rows, fr.counts, pq, pt, p, n_threads=8)
        n, _ = matcher.all_vs_all_plan()
        got, got2, sums = _bulk(matcher, pkg, n, pkg.capi.ROUTE_PACKED)
        np.testing.assert_array_equal(got, want, err_msg="2-byte words")
        np.testing.assert_array_equal(got2, want, err_msg="4-byte keys")
        np.testing.assert_array_equal(sums, wsums, err_msg="4-byte keys (index checksums)")
    finally:
        _restore(matcher, pkg)


ONLINE_SPECS = [("near", 33, 31), ("far", 65, 63, "tied"), ("near", 4, 4), ("far", 31, 33), ("near", 600, 130)]


def _online_cases(pkg):
    R = pkg.capi
    # (variant, LCM_TUNE_ONLINE_SPLIT, cross_check, route): the 600-row query is cut into 512-row chunks when split
    return [(0, 2, 0, R.ROUTE_SPLIT), (0, 0, 0, R.ROUTE_PLAIN), (4, -1, 0, R.ROUTE_MATRIX), (5, -1, 0, R.ROUTE_MATRIX),
            (0, -1, 1, R.ROUTE_CROSS), (0, -1, 2, R.ROUTE_CROSS)]


@pytest.mark.parametrize("ratio,floor", GRID)
def test_online_queries_every_route(matcher, oracle, pkg, ratio, floor):
    """lcm_query_scores, a micro-batch (lcm_query_submit_batch / collect_batch) and lcm_detect_loops of the last planted
    query frame (600 rows) and of a second query (the first pair's query rows under a new id) against the rest."""
    fr = planted.frames(ONLINE_SPECS, ratio, floor, seed=400, duplicate=False)
    n_db = fr.n_frames - 1
    last = fr.frame(n_db)
    qid = int(fr.ids[n_db])
    second = fr.frame(fr.pairs[0][0])
    try:
        _fill(matcher, fr, n_db)
        for variant, split, cross, route in _online_cases(pkg):
            matcher.set_params(ratio=ratio, dist_floor=floor, min_gap=1, min_matches=3, sim_threshold=0.0, cross_check=cross)
            matcher.set_kernel_variant(variant)
            matcher.set_tuning(pkg.capi.TUNE_ONLINE_SPLIT, split)
            p = oracle.default_params(ratio=ratio, dist_floor=floor, min_gap=1, min_matches=3, sim_threshold=0.0,
                                      cross_check=cross)
            want, _, woffs = _want_ext(oracle, fr, n_db, [last, second], [qid, qid + 1], p)
            tag = f"variant={variant} split={split} cross={cross}"
            s, sid = matcher.query_scores(last, qid)
            assert matcher.launch_info().route == route, tag
            np.testing.assert_array_equal(s, want[: woffs[1]], err_msg=tag)
            np.testing.assert_array_equal(sid, fr.ids[:n_db], err_msg=tag)
            t = matcher.query_submit_batch([last, second], [qid, qid + 1])
            sc, boffs = matcher.query_collect_batch(t)
            assert matcher.launch_info().route == route, tag + " (batch)"
            np.testing.assert_array_equal(sc, want, err_msg=tag + " (batch)")
            np.testing.assert_array_equal(boffs.astype(np.int64), woffs, err_msg=tag + " (batch)")
            c = matcher.detect_loops(qid, last)
            assert matcher.launch_info().route == route, tag + " (detect_loops)"
            expect = []
            for k in range(int(woffs[1])):
                ok, sim = oracle.loop_test(int(want[k]["good_count"]), len(last), int(fr.counts[k]), p)
                if ok:
                    expect.append((int(fr.ids[k]), int(want[k]["good_count"]), sim))
            got = [(int(x["matched_frame_id"]), int(x["num_matches"]), float(x["similarity_score"])) for x in c]
            assert got == expect, tag + " (detect_loops)"
    finally:
        _restore(matcher, pkg)


PAIR_SPECS = [("near", 65, 64), ("far", 33, 31, "tied"), ("near", 130, 130), ("far", 64, 63), ("near", 5, 1)]


@pytest.mark.parametrize("ratio,floor", GRID)
def test_pair_mode_match_lists(matcher, oracle, pkg, ratio, floor):
    """lcm_match_features, lcm_match_stored_batch and lcm_match_query_batch (host-side filter of the folded keys) under
    both LCM_TUNE_PAIR_HOST_FOLD settings; with dist_floor >= 256 the list is the whole BFMatcher.match list."""
    fr = planted.frames(PAIR_SPECS, ratio, floor, seed=500, empty=False, duplicate=False)
    p = oracle.default_params(ratio=ratio, dist_floor=floor)

    def same(got, want, tag):
        for f in ("query_idx", "train_idx", "img_idx", "distance"):
            np.testing.assert_array_equal(got[f], want[f].astype(got[f].dtype), err_msg=f"{tag}: {f}")

    try:
        _fill(matcher, fr)
        matcher.set_params(ratio=ratio, dist_floor=floor)
        for fold in (1, 0):
            matcher.set_tuning(pkg.capi.TUNE_PAIR_HOST_FOLD, fold)
            for c, t, _ in fr.pairs:
                q_rows, t_rows = fr.frame(c), fr.frame(t)
                want, wmd = oracle.match_features(q_rows, t_rows, p)
                got, md = matcher.match_features(q_rows, t_rows)
                assert md == wmd
                same(got, want, f"match_features fold={fold} pair {c},{t}")
                if floor >= 256:
                    oi, od = oracle.bf_match(q_rows, t_rows)
                    np.testing.assert_array_equal(got["query_idx"], np.arange(len(q_rows)))
                    np.testing.assert_array_equal(got["train_idx"], oi)
                    np.testing.assert_array_equal(got["distance"], od.astype(np.float32))
            pairs = [(int(fr.ids[c]), int(fr.ids[t])) for c, t, _ in fr.pairs]
            lists, mins = matcher.match_stored_batch(pairs)
            for (c, t, _), got, md in zip(fr.pairs, lists, mins):
                want, wmd = oracle.match_features(fr.frame(c), fr.frame(t), p)
                assert int(md) == wmd
                same(got, want, f"match_stored_batch fold={fold} pair {c},{t}")
            c0 = fr.pairs[0][0]
            train_ids = [int(fr.ids[t]) for t in range(fr.n_frames)]
            lists, mins = matcher.match_query_batch(fr.frame(c0), train_ids)
            for t, got, md in zip(range(fr.n_frames), lists, mins):
                want, wmd = oracle.match_features(fr.frame(c0), fr.frame(t), p)
                assert int(md) == wmd
                same(got, want, f"match_query_batch fold={fold} train {t}")
    finally:
        _restore(matcher, pkg)


def test_loopback_group_takes_the_parameters_to_every_shard(pkg, oracle):
    """W = 3 shards on one device: lcm_group_set_params, then bulk records, argmin records + checksums and an online
    query == the oracle at every grid point (a shard left on the old parameters would differ on its third of the pairs)."""
    with pkg.Group(pkg.default_params(), n_devices=3, loopback_device=0) as g:
        for ratio, floor in GRID:
            fr = planted.frames(SPECS[:7], ratio, floor, seed=600)
            params = pkg.default_params()
            params.ratio, params.dist_floor, params.min_gap = ratio, floor, 1
            g.set_params(params)
            g.clear()
            for f in range(fr.n_frames - 1):
                g.append(int(fr.ids[f]), fr.frame(f))
            p = oracle.default_params(ratio=ratio, dist_floor=floor, min_gap=1)
            n_db = fr.n_frames - 1
            pq, pt = _self_pairs(fr.ids[:n_db])
            want, wsums = oracle.fast_score_pairs_idx(fr.rows[:n_db], fr.counts[:n_db], pq, pt, p, n_threads=8)
            tag = f"ratio={ratio} floor={floor}"
            s, _ = g.all_vs_all()
            np.testing.assert_array_equal(s, want, err_msg=tag)
            s2, sums, _ = g.all_vs_all_argmin()
            np.testing.assert_array_equal(s2, want, err_msg=tag + " (argmin)")
            np.testing.assert_array_equal(sums, wsums, err_msg=tag + " (index checksums)")
            q = fr.frame(n_db)
            qs, qids = g.query_scores(q, int(fr.ids[n_db]))
            wq, _, _ = _want_ext(oracle, fr, n_db, [q], [int(fr.ids[n_db])], p)
            np.testing.assert_array_equal(qs, wq, err_msg=tag + " (query_scores)")
            np.testing.assert_array_equal(qids, fr.ids[:n_db])

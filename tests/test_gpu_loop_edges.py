"""The loop test `den = min(kp_q, kp_t) > 0 and good >= min_matches and (double)good / (double)den > sim_threshold` on
every route that forms the verdict, with pairs placed exactly ON its edges (tests/loopcases.py): planted revisits at the
default parameters (49 / 50 / 51 matches, 300 / 2000 == 0.15 exactly, 301 / 2000, the `min` of the two keypoint counts,
a zero count on either side, similarity 1.0 and above) and parameter sets taken from the oracle's own scores of pairs
that sit on the wave and block seams of the compaction kernels (min_matches = G / G + 1, sim_threshold = G / D and the
double just below, all / none).

Routes: the fused device search (`loop_verdict` in k_loop_count / k_loop_emit, self and external query sets, every
kernel variant and packed mode, the block scan's carry above 1024 blocks), lcm_detect_loops (host rows with and without a
keypoint count, stored frame, stored frame above 2048 rows, split / unsplit regimes), the group's two routes (W = 1 and a W = 3
loopback, parameters changed on the live group), the host class (single handle and group) and parameter changes on the
session matcher without an append in between.  Every expected list is `loopcases.expected` — plain Python over the
oracle's records; candidates are compared field by field, similarities with ==."""
import ctypes as C
import math

import numpy as np
import pytest

import loopcases as L

pytestmark = pytest.mark.gpu

D = L.DEFAULT


def _restore(matcher, pkg):
    matcher.set_params(ratio=2, dist_floor=0, min_gap=30, min_matches=50, sim_threshold=0.15, cross_check=0)
    matcher.set_kernel_variant(0)
    matcher.set_tuning(pkg.capi.TUNE_PACKED, -1)
    matcher.set_tuning(pkg.capi.TUNE_ONLINE_SPLIT, -1)
    matcher.clear()


def _fill(m, ls, give_kp=True):
    m.clear()
    for f in range(ls.n_frames):
        m.append(int(ls.ids[f]), ls.frame(f), int(ls.kp[f]) if give_kp else -1)


def _by_rows(ls):
    """The same set with the row counts as keypoint counts (what n_keypoints = -1 means)."""
    return L.LoopSet(ls.rows, ls.counts, ls.ids, ls.counts, ls.gap, [], ls.pq, ls.pt, ls.offs, ls.good)


def _fused(matcher, ls, mm, thr, tag="", **ext):
    matcher.set_params(min_matches=mm, sim_threshold=thr, min_gap=ls.gap)
    cands, npairs = matcher.all_vs_all_loops(cap=len(ls.pq), **ext)
    assert npairs == len(ls.pq), tag
    return L.as_tuples(cands)


def _params(pkg, mm, thr, gap):
    p = pkg.default_params()
    p.min_matches, p.sim_threshold, p.min_gap = mm, thr, gap
    return p


# ---------------------------------------------------------------------------------------------------------------------
# fused device search
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_search_planted_edges_at_the_defaults(matcher, oracle, pkg):
    ls = L.planted(oracle)
    want = L.expected(ls, D["min_matches"], D["sim_threshold"])
    try:
        _fill(matcher, ls)
        assert matcher.params.min_matches == 50 and matcher.params.sim_threshold == 0.15 and matcher.params.min_gap == 30
        cands, npairs = matcher.all_vs_all_loops(cap=len(ls.pq))
        assert npairs == len(ls.pq)
        assert L.as_tuples(cands) == want
        # one below the count: LCM_ERR_CAPACITY, and the count is reported
        lib = pkg.load_library()
        out = np.zeros(len(want), pkg.capi.CANDIDATE_DTYPE)
        n, npairs = C.c_size_t(0), C.c_size_t(0)
        rc = lib.lcm_all_vs_all_loops(matcher._h, None, None, None, None, len(matcher), 0, out.ctypes.data_as(C.c_void_p),
                                      len(want) - 1, C.byref(n), C.byref(npairs))
        assert rc == pkg.capi.ERR_CAPACITY and n.value == len(want)
        # the row counts as denominators (appended without a keypoint count): another list
        _fill(matcher, ls, give_kp=False)
        by_rows = L.expected(_by_rows(ls), D["min_matches"], D["sim_threshold"])
        assert by_rows != want
        cands, _ = matcher.all_vs_all_loops(cap=len(ls.pq))
        assert L.as_tuples(cands) == by_rows
    finally:
        _restore(matcher, pkg)


def test_fused_search_every_derived_parameter_set(matcher, oracle, pkg):
    """One database, 34 parameter sets, no append in between: each target pair flips between its two sets."""
    ls, targets, sets = L.derived(oracle, pkg)
    try:
        _fill(matcher, ls)
        for mm, thr in sets:
            assert _fused(matcher, ls, mm, thr) == L.expected(ls, mm, thr), (mm, thr)
    finally:
        _restore(matcher, pkg)


def test_fused_search_only_the_seam_pairs_pass(matcher, oracle, pkg):
    """Sparse: the only candidates sit at pair 0, 63 / 64 (wave edge), 255 / 256 / 257 (block edge), the last pair of a
    query frame, the first of the next and the last pair; dense: every lane of every wave passes."""
    ls, positions = L.seams(oracle)
    try:
        _fill(matcher, ls)
        got = _fused(matcher, ls, 2, -1.0)
        assert got == L.expected(ls, 2, -1.0) and len(got) == len(positions)
        got = _fused(matcher, ls, 0, -1.0)
        assert got == L.expected(ls, 0, -1.0) and len(got) == len(ls.pq)
        got = _fused(matcher, ls, 3, 0.25)                       # 3 / 12 == 0.25 exactly: strict, none
        assert got == L.expected(ls, 3, 0.25) == []
        got = _fused(matcher, ls, 3, math.nextafter(0.25, 0.0))
        assert got == L.expected(ls, 3, math.nextafter(0.25, 0.0)) and len(got) == len(positions)
    finally:
        _restore(matcher, pkg)


def test_fused_search_external_query_set_and_its_keypoints(matcher, oracle, pkg):
    """The same frames as an external query set: q_keypoints given (the planted counts, one of them negative, and counts
    that are neither the stored ones nor the row counts), then q_keypoints = NULL (the query ROW counts are the
    denominators: another list)."""
    ds, targets, _ = L.derived(oracle, pkg)
    _, G, Dn = targets[2]
    for ls, psets in ((L.planted(oracle), [(D["min_matches"], D["sim_threshold"])]),
                      (ds, [(0, G / Dn), (0, math.nextafter(G / Dn, -math.inf)), (G, 0.9)])):
        q_counts = ls.counts.astype(np.int32)
        d_rows, d_counts = matcher.dev_alloc(ls.rows.nbytes), matcher.dev_alloc(q_counts.nbytes)
        try:
            matcher.clear()
            for f in range(ls.n_frames):                          # stored side: kp as planted
                matcher.append(int(ls.ids[f]), ls.frame(f), int(ls.kp[f]))
            matcher.dev_upload(d_rows, ls.rows); matcher.dev_upload(d_counts, q_counts)
            ext = dict(d_query_rows=d_rows, d_query_counts=d_counts, q_ids=ls.ids, q_stride_rows=ls.rows.shape[1])
            q_kp = ls.kp.copy()
            q_kp[ls.n_frames - 2] = -5                            # a negative count handed in: never a loop
            odd = ls.kp + 1                                       # neither the stored counts nor the row counts
            odd[ls.kp == 0] = 0
            for mm, thr in psets:
                for kps, tag in ((ls.kp, "q_keypoints == stored"), (q_kp, "a negative q_keypoints"), (odd, "kp + 1")):
                    got = _fused(matcher, ls, mm, thr, tag, q_keypoints=kps, **ext)
                    assert got == L.expected(ls, mm, thr, q_kp=kps), (tag, mm, thr)
                got = _fused(matcher, ls, mm, thr, "NULL", **ext)
                assert got == L.expected(ls, mm, thr, q_kp=ls.counts), ("q_keypoints NULL", mm, thr)
            mm, thr = psets[0]
            assert L.expected(ls, mm, thr, q_kp=ls.counts) != L.expected(ls, mm, thr) != L.expected(ls, mm, thr, q_kp=odd)
        finally:
            matcher.dev_free(d_rows); matcher.dev_free(d_counts)
            _restore(matcher, pkg)


def test_fused_search_every_kernel_variant_and_packed_mode(matcher, oracle, pkg):
    """The verdict kernels are the same, the score array they read is written by another kernel each time."""
    ls, targets, sets = L.derived(oracle, pkg)
    R = pkg.capi
    cases = [(0, 0, R.ROUTE_PLAIN), (1, 0, R.ROUTE_PLAIN), (2, 0, R.ROUTE_PLAIN), (3, 0, R.ROUTE_PLAIN),
             (4, 0, R.ROUTE_MATRIX), (5, 0, R.ROUTE_MATRIX), (0, 1, R.ROUTE_PACKED), (0, 2, R.ROUTE_PACKED),
             (0, -1, None)]
    try:
        _fill(matcher, ls)
        for k, (variant, packed, route) in enumerate(cases):
            matcher.set_kernel_variant(variant)
            matcher.set_tuning(R.TUNE_PACKED, packed)
            _, G, Dn = targets[k]
            for mm, thr in ((0, G / Dn), (0, math.nextafter(G / Dn, -math.inf))):
                got = _fused(matcher, ls, mm, thr)
                if route is not None:
                    assert matcher.launch_info().route == route, (variant, packed)
                assert got == L.expected(ls, mm, thr), (variant, packed, mm, thr)
        ps = L.planted(oracle)                                          # and the planted set where it is admitted
        _fill(matcher, ps)
        matcher.set_kernel_variant(0)
        for packed in (1, 2, -1):
            matcher.set_tuning(R.TUNE_PACKED, packed)
            assert _fused(matcher, ps, D["min_matches"], D["sim_threshold"]) == \
                L.expected(ps, D["min_matches"], D["sim_threshold"]), packed
    finally:
        _restore(matcher, pkg)


def _cand_array(pkg, tuples):
    out = np.zeros(len(tuples), pkg.capi.CANDIDATE_DTYPE)
    if tuples:
        cur, mat, num, sim = zip(*tuples)
        out["current_frame_id"], out["matched_frame_id"], out["num_matches"], out["similarity_score"] = cur, mat, num, sim
    return out


def test_block_scan_carry_above_1024_blocks(matcher, oracle, pkg):
    """319,600 pairs = 1,249 blocks of 256: the scan runs a second 1024-entry chunk on top of the first one's carry.
    Dense (every block full) and sparse (keypoint counts: 2 % of the pairs, on both sides of pair 262,144)."""
    ls = L.scan(oracle, pkg)
    try:
        _fill(matcher, ls)
        for mm, thr in ((0, -1.0), L.SCAN_SPARSE, (4, 0.004), (0, 1.0)):
            want = _cand_array(pkg, L.expected(ls, mm, thr))
            matcher.set_params(min_matches=mm, sim_threshold=thr, min_gap=1)
            cands, npairs = matcher.all_vs_all_loops(cap=len(ls.pq))
            assert npairs == len(ls.pq) == 319600
            assert len(cands) == len(want), (mm, thr)
            for f in ("current_frame_id", "matched_frame_id", "num_matches", "similarity_score"):
                np.testing.assert_array_equal(cands[f], want[f], err_msg=f"{f} at {(mm, thr)}")
    finally:
        _restore(matcher, pkg)


# ---------------------------------------------------------------------------------------------------------------------
# online: lcm_detect_loops
# ---------------------------------------------------------------------------------------------------------------------
def _detect_all(m, ls, mode):
    got = []
    for f in range(ls.n_frames):
        if mode == "stored":
            c = m.detect_loops(int(ls.ids[f]))
        elif mode == "given":
            c = m.detect_loops(int(ls.ids[f]), ls.frame(f), int(ls.kp[f]))
        else:
            c = m.detect_loops(int(ls.ids[f]), ls.frame(f))
        got += L.as_tuples(c)
    return got


def test_detect_loops_planted_edges_every_query_form(matcher, oracle, pkg):
    """Host rows with n_keypoints given, host rows with -1 (the row count), the stored frame (its stored count); the
    2100-row frame goes through each, as host rows and as a stored frame above 2048 rows."""
    ls = L.planted(oracle)
    mm, thr = D["min_matches"], D["sim_threshold"]
    want = L.expected(ls, mm, thr)
    want_rows = L.expected(ls, mm, thr, q_kp=ls.counts)           # query side by rows, stored side as appended
    assert want != want_rows
    big = int(np.argmax(ls.counts))
    q2000 = next(c for c, _, _ in ls.planted if ls.counts[c] == 2000)
    assert ls.counts[big] > 2048 and any(c == int(ls.ids[big]) for c, *_ in want)
    try:
        _fill(matcher, ls)
        for split in (-1, 2, 0):
            matcher.set_tuning(pkg.capi.TUNE_ONLINE_SPLIT, split)
            assert _detect_all(matcher, ls, "given") == want, split
            assert _detect_all(matcher, ls, "rows") == want_rows, split
            assert _detect_all(matcher, ls, "stored") == want, split
            if split >= 0:                                    # a 2000-row query is cut into 512-row chunks, or is not
                matcher.detect_loops(int(ls.ids[q2000]), ls.frame(q2000), int(ls.kp[q2000]))
                assert matcher.launch_info().route == (pkg.capi.ROUTE_SPLIT if split else pkg.capi.ROUTE_PLAIN)
    finally:
        _restore(matcher, pkg)


def test_detect_loops_every_derived_parameter_set(matcher, oracle, pkg):
    """(Frames of at most 512 rows are never cut into chunks: the split regimes are the planted set's, above.)"""
    ls, targets, sets = L.derived(oracle, pkg)
    try:
        _fill(matcher, ls)
        for k, (mm, thr) in enumerate(sets):
            matcher.set_params(min_matches=mm, sim_threshold=thr, min_gap=1)
            assert _detect_all(matcher, ls, "given") == L.expected(ls, mm, thr), (mm, thr)
            if k % 4 == 2:
                assert _detect_all(matcher, ls, "stored") == L.expected(ls, mm, thr), (mm, thr)
                assert _detect_all(matcher, ls, "rows") == L.expected(ls, mm, thr, q_kp=ls.counts), (mm, thr)
    finally:
        _restore(matcher, pkg)


# ---------------------------------------------------------------------------------------------------------------------
# groups: the fused search reads the SHARDS' parameters and per-shard keypoint lists, detect_loops reads the group's
# ---------------------------------------------------------------------------------------------------------------------
def _group_detect_all(g, ls, give_kp=True):
    got = []
    for f in range(ls.n_frames):
        got += L.as_tuples(g.detect_loops(int(ls.ids[f]), ls.frame(f), int(ls.kp[f]) if give_kp else -1))
    return got


@pytest.mark.parametrize("world", [1, 3])
def test_group_routes_and_parameter_changes_on_a_live_group(pkg, oracle, world):
    """W = 1 is an RCCL communicator of one, W = 3 a loopback group.  The derived set's keypoint counts are all distinct:
    a shard-local / global slot mix-up in the per-shard keypoint list changes the answer."""
    ps = L.planted(oracle)
    ds, targets, sets = L.derived(oracle, pkg)
    kw = dict(n_devices=1) if world == 1 else dict(n_devices=world, loopback_device=0)
    mm0, thr0 = D["min_matches"], D["sim_threshold"]
    with pkg.Group(pkg.default_params(), **kw) as g:
        assert g.world == world
        for f in range(ps.n_frames):
            g.append(int(ps.ids[f]), ps.frame(f), int(ps.kp[f]))
        want = L.expected(ps, mm0, thr0)
        cands, npairs = g.all_vs_all_loops(cap=len(ps.pq))
        assert npairs == len(ps.pq) and L.as_tuples(cands) == want
        assert _group_detect_all(g, ps) == want
        assert _group_detect_all(g, ps, give_kp=False) == L.expected(ps, mm0, thr0, q_kp=ps.counts) != want
        # LCM_ERR_CAPACITY with the count
        out = np.zeros(len(want) - 1, pkg.capi.CANDIDATE_DTYPE)
        with pytest.raises(pkg.capi.LcmError) as e:
            g.all_vs_all_loops(out=out)
        assert e.value.code == pkg.capi.ERR_CAPACITY
        # a planted quotient as threshold on the live group: 301 / 2000 leaves, and comes back one double below
        q = 301 / 2000
        for thr in (q, math.nextafter(q, 0.0), thr0):
            g.set_params(_params(pkg, mm0, thr, 30))
            w = L.expected(ps, mm0, thr)
            assert L.as_tuples(g.all_vs_all_loops(cap=len(ps.pq))[0]) == w, thr
            assert _group_detect_all(g, ps) == w, thr
        assert len(L.expected(ps, mm0, q)) < len(L.expected(ps, mm0, math.nextafter(q, 0.0)))
        # the derived set and its parameter sets, changed on the live group; then back
        g.set_params(_params(pkg, mm0, thr0, 1))
        g.clear()
        for f in range(ds.n_frames):
            g.append(int(ds.ids[f]), ds.frame(f), int(ds.kp[f]))
        w = L.expected(ds, mm0, thr0)
        assert L.as_tuples(g.all_vs_all_loops(cap=len(ds.pq))[0]) == w and len(w) > 0
        for mm, thr in sets[: 16 if world == 3 else 8] + [(mm0, thr0)]:
            g.set_params(_params(pkg, mm, thr, 1))
            w = L.expected(ds, mm, thr)
            cands, npairs = g.all_vs_all_loops(cap=len(ds.pq))
            assert npairs == len(ds.pq) and L.as_tuples(cands) == w, (mm, thr)
            assert _group_detect_all(g, ds) == w, (mm, thr)
        # refused parameters leave every shard AND the group on the old ones
        bad = _params(pkg, mm0, math.nan, 1)
        with pytest.raises(pkg.capi.LcmError):
            g.set_params(bad)
        w = L.expected(ds, mm0, thr0)
        assert L.as_tuples(g.all_vs_all_loops(cap=len(ds.pq))[0]) == w
        assert _group_detect_all(g, ds) == w


# ---------------------------------------------------------------------------------------------------------------------
# host class: loop_threshold and the gap only (min_matches stays 50), so the planted set carries it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [0, 3])
def test_host_class_planted_edges(pkg, oracle, shards):
    ls = L.planted(oracle)
    q = 301 / 2000
    assert q != 0.15 and L.expected(ls, 50, q) != L.expected(ls, 50, 0.15)
    revisits = sorted({c for c, _, _ in ls.planted})
    for thr in (0.15, q, math.nextafter(q, 0.0)):
        want = L.expected(ls, 50, thr)
        one = pkg.LoopClosingSystem(thr, 30, loopback_shards=shards)
        many = pkg.LoopClosingSystem(thr, 30, loopback_shards=shards)
        try:
            for f in range(ls.n_frames):
                one.processFrame(ls.frame(f), int(ls.ids[f]), int(ls.kp[f]))
            assert L.as_tuples(one.getLoopClosures()) == want, thr
            for a in range(0, ls.n_frames, 5):
                fr = range(a, min(a + 5, ls.n_frames))
                many.processFrames([ls.frame(f) for f in fr], [int(ls.ids[f]) for f in fr], [int(ls.kp[f]) for f in fr])
            assert L.as_tuples(many.getLoopClosures()) == want, thr
            for s in (one, many):
                got = [x for c in revisits for x in L.as_tuples(s.detectLoops(int(ls.ids[c])))]
                assert got == [w for c in revisits for w in L.expected(ls, 50, thr, only_query=c)], thr
        finally:
            one.close(); many.close()


# ---------------------------------------------------------------------------------------------------------------------
# lcm_set_params: takes effect on the next search without an append (plan reuse); its argument rules
# ---------------------------------------------------------------------------------------------------------------------
def test_set_params_between_two_calls_and_its_argument_rules(matcher, oracle, pkg):
    ls, targets, sets = L.derived(oracle, pkg)
    _, G, Dn = targets[3]
    cur = ls.pq[targets[3][0]]
    lib = pkg.load_library()
    try:
        _fill(matcher, ls)
        for mm, thr in ((G, -1.0), (G + 1, -1.0), (0, G / Dn), (0, math.nextafter(G / Dn, -math.inf)), (G, -1.0)):
            matcher.set_params(min_matches=mm, sim_threshold=thr, min_gap=1)          # no append from here on
            cands, _ = matcher.all_vs_all_loops(cap=len(ls.pq))
            assert L.as_tuples(cands) == L.expected(ls, mm, thr), (mm, thr)
            assert L.as_tuples(matcher.detect_loops(int(ls.ids[cur]))) == L.expected(ls, mm, thr, only_query=cur)
            assert L.as_tuples(matcher.detect_loops(int(ls.ids[cur]), ls.frame(cur), int(ls.kp[cur]))) == \
                L.expected(ls, mm, thr, only_query=cur)
        # refused: NaN threshold, negative min_matches; the old parameters stay in force
        before = L.expected(ls, G, -1.0)
        for field, value in (("sim_threshold", math.nan), ("min_matches", -1)):
            p = matcher.params
            setattr(p, field, value)
            assert lib.lcm_set_params(matcher._h, C.byref(p)) == pkg.capi.ERR_INVALID_ARG, field
            now = matcher.params
            assert now.min_matches == G and now.sim_threshold == -1.0 and now.min_gap == 1
            assert L.as_tuples(matcher.all_vs_all_loops(cap=len(ls.pq))[0]) == before
        # accepted: negative and infinite thresholds
        for thr in (-0.5, -math.inf, math.inf):
            matcher.set_params(min_matches=0, sim_threshold=thr, min_gap=1)
            assert matcher.params.sim_threshold == thr
            got = L.as_tuples(matcher.all_vs_all_loops(cap=len(ls.pq))[0])
            assert got == L.expected(ls, 0, thr) and len(got) == (0 if thr == math.inf else len(ls.pq))
            assert L.as_tuples(matcher.detect_loops(int(ls.ids[cur]))) == L.expected(ls, 0, thr, only_query=cur)
    finally:
        _restore(matcher, pkg)

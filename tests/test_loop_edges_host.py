"""The loop test's boundaries on the routes that need no device: the generators of tests/loopcases.py (their own
assertions, and that they notice a lost edge), the pure-Python reference == oracle.loop_test == oracle.detect_loops,
the host C function lcm_loop_test over the whole grid, and sharding.ShardedLoopSearch with an oracle scorer."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import loopcases as L

D = L.DEFAULT


def _oparams(oracle, mm, thr, gap):
    return oracle.default_params(min_matches=mm, sim_threshold=thr, min_gap=gap)


def test_generators_hold_every_edge_they_promise(oracle, pkg):
    ls = L.planted(oracle)
    assert L.check_planted(ls)
    assert len(ls.planted) == len(L.PLANTED_SPECS) and ls.n_frames == 28
    assert max(ls.counts) > 2048 and list(ls.counts).count(2000) >= 4
    ds, targets, sets = L.derived(oracle, pkg)
    assert len(targets) == 9 and len(sets) >= 30
    ss, positions = L.seams(oracle)
    assert {0, 63, 64, 255, 256, 257, len(ss.pq) - 1} <= set(positions)
    sc = L.scan(oracle, pkg)
    assert len(sc.pq) == 319600


@pytest.mark.parametrize("frame,new_kp,edge", [(4, 1998, "300 / 2000 == 0.15 exactly"), (24, 5, "query kp 0"),
                                               (26, 149, "similarity exactly 1.0")])
def test_generator_notices_a_lost_edge(oracle, frame, new_kp, edge):
    """One keypoint count changed: the set no longer holds that edge and its own check says so."""
    import copy
    ls = copy.copy(L.planted(oracle))
    ls.kp = ls.kp.copy()
    ls.kp[frame] = new_kp
    with pytest.raises(AssertionError, match=re.escape("lost the edge: " + edge)):
        L.check_planted(ls)
    ls = copy.copy(L.planted(oracle))          # and a planted pair whose count is off by one
    ls.good = list(ls.good)
    ls.good[ls.pair_index(*ls.planted[1][:2])] += 1
    with pytest.raises(AssertionError, match="intended 50"):
        L.check_planted(ls)


def test_reference_is_the_oracle_loop_test_pair_by_pair(oracle, pkg):
    ps = L.planted(oracle)
    ds, _, sets = L.derived(oracle, pkg)
    for ls, psets in ((ps, [(D["min_matches"], D["sim_threshold"])] + sets[:8]), (ds, sets)):
        ids = [int(i) for i in ls.ids]
        for mm, thr in psets:
            p = _oparams(oracle, mm, thr, ls.gap)
            want = []
            for c, t, g in zip(ls.pq, ls.pt, ls.good):
                ok, sim = oracle.loop_test(g, int(ls.kp[c]), int(ls.kp[t]), p)
                den = min(int(ls.kp[c]), int(ls.kp[t]))
                assert sim == (g / den if den > 0 else 0.0)
                if ok:
                    want.append((ids[c], ids[t], g, sim))
            assert L.expected(ls, mm, thr) == want, (mm, thr)


def test_reference_is_oracle_detect_loops_where_keypoints_are_rows(oracle):
    """orc_detect_loops takes the row counts as keypoint counts: the seam set (kp == rows) frame by frame, and the
    planted set's small frames with their row counts."""
    ss, _ = L.seams(oracle)
    p = _oparams(oracle, 2, -1.0, 1)
    got = [x for cur in range(ss.n_frames) for x in L.as_tuples(oracle.detect_loops(ss.rows, ss.counts, ss.ids, cur, p))]
    assert got == L.expected(ss, 2, -1.0) and len(got) == 9
    ps = L.planted(oracle)
    p = _oparams(oracle, D["min_matches"], D["sim_threshold"], D["min_gap"])
    for cur in (15, 18, 25, 26, 27):                     # 180 / 70 / 95 / 150 / 77 rows: cheap for the scalar oracle
        small = [f for f in range(ps.n_frames) if ps.counts[f] <= 513]
        k = small.index(cur)
        sub = L.LoopSet(ps.rows[small, :513], ps.counts[small], ps.ids[small], ps.counts[small], ps.gap)
        L._score(oracle, sub)
        got = L.as_tuples(oracle.detect_loops(sub.rows, sub.counts, sub.ids, k, p))
        assert got == L.expected(sub, D["min_matches"], D["sim_threshold"], only_query=k)


def _loop_test(lib, pkg, mm, thr, good, kq, kt, want_sim=True):
    p = pkg.default_params()
    p.min_matches, p.sim_threshold = mm, thr
    s = pkg.capi.Score(good, 0, 0)
    sim = C.c_double(-7.0)
    r = lib.lcm_loop_test(C.byref(p), C.byref(s), kq, kt, C.byref(sim) if want_sim else None)
    return r, sim.value


def test_lcm_loop_test_over_the_whole_grid(oracle, pkg):
    """The host C function (loads without a device) == the reference: verdict and written similarity."""
    lib = pkg.load_library()

    def ref(mm, thr, g, kq, kt):
        den = min(kq, kt)
        return (1 if den > 0 and g >= mm and g / den > thr else 0), (g / den if den > 0 else 0.0)

    ps = L.planted(oracle)
    ds, _, sets = L.derived(oracle, pkg)
    n = 0
    for ls, psets in ((ps, [(D["min_matches"], D["sim_threshold"])] + sets), (ds, sets)):
        for mm, thr in psets:
            for c, t, g in zip(ls.pq, ls.pt, ls.good):
                kq, kt = int(ls.kp[c]), int(ls.kp[t])
                assert _loop_test(lib, pkg, mm, thr, g, kq, kt) == ref(mm, thr, g, kq, kt), (mm, thr, g, kq, kt)
                n += 1
    assert n > 50000
    # the planted edges by hand, at the defaults
    for g, kq, kt, verdict in [(49, 333, 333, 0), (50, 333, 333, 1), (51, 333, 333, 1), (49, 100, 100, 0),
                               (300, 2000, 2000, 0), (301, 2000, 2000, 1), (300, 2000, 1999, 1), (300, 1999, 2000, 1),
                               (60, 0, 75, 0), (60, 95, 0, 0), (150, 150, 150, 1), (77, 76, 77, 1)]:
        r, sim = _loop_test(lib, pkg, 50, 0.15, g, kq, kt)
        assert (r, sim) == ref(50, 0.15, g, kq, kt) and r == verdict, (g, kq, kt)
    assert _loop_test(lib, pkg, 50, 0.15, 150, 150, 150)[1] == 1.0
    assert _loop_test(lib, pkg, 50, 0.15, 300, 2000, 2000)[1] == 0.15
    # zero and negative keypoint counts: never a loop, similarity 0.0, whatever the threshold
    for kq, kt in [(0, 0), (0, 5), (5, 0), (-1, 5), (5, -1), (-3, -2), (-2 ** 31, 7)]:
        for mm, thr in [(0, -1.0), (0, -math.inf), (50, 0.15)]:
            assert _loop_test(lib, pkg, mm, thr, 60, kq, kt) == (0, 0.0), (kq, kt, mm, thr)
    # good_count is unsigned 32-bit, min_matches signed: 2**32 - 1 matches pass min_matches = 2**31 - 1
    big = 2 ** 32 - 1
    assert _loop_test(lib, pkg, L.INT_MAX, -1.0, big, 10, 10) == (1, big / 10)
    assert _loop_test(lib, pkg, L.INT_MAX, -1.0, L.INT_MAX - 1, 10, 10) == (0, (L.INT_MAX - 1) / 10)
    assert _loop_test(lib, pkg, L.INT_MAX, -1.0, L.INT_MAX, 10, 10)[0] == 1
    assert _loop_test(lib, pkg, 0, math.inf, big, 1, 1)[0] == 0
    # a NULL similarity pointer changes no verdict
    for g, kq, kt in [(50, 333, 333), (49, 333, 333), (300, 2000, 2000), (301, 2000, 2000), (60, 0, 9)]:
        assert _loop_test(lib, pkg, 50, 0.15, g, kq, kt, want_sim=False)[0] == ref(50, 0.15, g, kq, kt)[0]


class _OracleScorer:
    """CPU stand-in for Matcher (as in test_sharding_gloo.py): same interface, records from the oracle."""

    def __init__(self, oracle, params):
        self.oracle, self.params, self.frames = oracle, params, []

    def __len__(self):
        return len(self.frames)

    def append(self, frame_id, rows, n_keypoints=-1):
        self.frames.append((int(frame_id), np.ascontiguousarray(rows)))

    def query_scores(self, rows, frame_id):
        gap = max(int(self.params.min_gap), 1)
        el = [(i, r) for i, r in self.frames if frame_id - i >= gap]
        stride = max([len(rows)] + [len(r) for _, r in el] + [1])
        buf = np.zeros((len(el) + 1, stride, 32), np.uint8)
        buf[0, : len(rows)] = rows
        for k, (_, r) in enumerate(el):
            buf[k + 1, : len(r)] = r
        counts = np.array([len(rows)] + [len(r) for _, r in el], np.int32)
        sc, _, _ = self.oracle.fast_score_pairs(buf, counts, [0] * len(el), list(range(1, len(el) + 1)), self.params,
                                                n_threads=8)
        return sc, np.array([i for i, _ in el], np.int32)


def test_sharded_loop_search_driver(oracle, pkg):
    """sharding.ShardedLoopSearch.process_frame restates the loop test in Python: planted set at the defaults (keypoint
    counts given), two derived sets, and the n_keypoints = -1 default (row counts)."""
    ps = L.planted(oracle)
    ds, targets, sets = L.derived(oracle, pkg)
    _, G, Dn = targets[1]
    cases = [(ps, D["min_matches"], D["sim_threshold"], True), (ps, D["min_matches"], D["sim_threshold"], False),
             (ds, 0, G / Dn, True), (ds, 0, math.nextafter(G / Dn, -math.inf), True), (ds, G + 1, -1.0, True)]
    for ls, mm, thr, give_kp in cases:
        p = _oparams(oracle, mm, thr, ls.gap)
        search = pkg.sharding.ShardedLoopSearch(_OracleScorer(oracle, p), 0, 1)
        got = []
        for f in range(ls.n_frames):
            _, _, cands = search.process_frame(ls.frame(f), int(ls.ids[f]), int(ls.kp[f]) if give_kp else -1)
            got += cands
        if give_kp:
            assert got == L.expected(ls, mm, thr), (mm, thr)
        else:
            by_rows = L.LoopSet(ls.rows, ls.counts, ls.ids, ls.counts, ls.gap, [], ls.pq, ls.pt, ls.offs, ls.good)
            assert got == L.expected(by_rows, mm, thr) != L.expected(ls, mm, thr)

"""The size envelope of include/lcm.h on the routes with TWO neighbours per query row: the Hamming k = 2 pair mode
(lcm_knn2_pair, lcm_match_*_ratio) and the ratio-scored bulk, online and loop searches (lcm_all_vs_all_ratio,
lcm_query_scores_ratio, lcm_detect_loops_ratio, lcm_all_vs_all_loops_ratio, the group forms) against 65535-row stored
frames, 65535-row queries, 2^22 train rows, 4096 / 8192 eligible frames in the online call and more than 2^20 work items in
the bulk call.  Inputs and what they plant: tests/knnlimitcases.py.  Expected values come from knnref / ratioref /
ratioloopref and plain numpy scans only; the k = 1 result and lcm_last_bulk_scores are second witnesses.

References are module-scoped and computed once (knnref.knn2 in 512-row blocks on a few threads).  Every test that owns a
handle frees it in `finally`; nothing is retried."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import knnlimitcases as K
import knnref
import ratioloopref as R
import ratioref

pytestmark = pytest.mark.gpu

RATIOS = (0.7, 0.75, 1.0)
FIELDS = ("query_idx", "train_idx", "img_idx", "distance")
STORED_PAIRS = [("X", "A")] + [(s, t) for s in ("Y", "Z") for t in K.TALL]      # the pair-mode lists: X against A only
ALL_PAIRS = [(s, t) for s in K.SMALL for t in K.TALL]                            # the ratio search: all 9 eligible pairs


def knn2_threads(jobs, threads=6):
    """{key: knnref.knn2(q, t)} for jobs {key: (q, t)}, in blocks of 512 query rows spread over a few threads (numpy
    releases the GIL inside its loops; a block against 65535 train rows holds ~0.4 GB for a moment)."""
    parts = [(key, r0) for key, (q, t) in jobs.items() for r0 in range(0, len(q), 512)]
    with ThreadPoolExecutor(threads) as ex:
        done = list(ex.map(lambda kr: knnref.knn2(jobs[kr[0]][0][kr[1]: kr[1] + 512], jobs[kr[0]][1]), parts))
    out = {}
    for key in jobs:
        mine = [d for (k, _), d in zip(parts, done) if k == key]
        out[key] = (np.concatenate([i for i, _ in mine]), np.concatenate([d for _, d in mine]))
    return out


@pytest.fixture(scope="module")
def tall():
    return K.full_tall_set()


@pytest.fixture(scope="module")
def refs(tall):
    """knnMatch(k = 2) of every eligible (small, tall) pair, of the small frames among themselves, of A's planted and 512
    sampled rows against B, and of A against the 33- and 513-row matrices: computed once, never changed."""
    fr = tall.frames
    rng = np.random.default_rng(77)
    sample = sorted(set(K.TQ_ROWS) | set(int(x) for x in rng.choice(65535, 512, replace=False)))
    cases = {nt: K.tall_query_case(tall, nt) for nt in (33, 513)}
    jobs = {(s, t): (fr[s], fr[t]) for s, t in ALL_PAIRS}
    jobs.update({(s, t): (fr[s], fr[t]) for s in K.SMALL for t in K.SMALL})
    jobs["AxB"] = (fr["A"][sample], fr["B"])
    for nt, c in cases.items():
        jobs[nt] = (c.query, c.train)
    out = knn2_threads(jobs)
    out["sample"], out["cases"] = np.array(sample), cases
    for t in K.TALL:                                # the trap, on the reference: best = last row at 0, a far second, all pass
        assert K.trap_expect(tall, t, *out[("Y", t)], 0.7) == 64
    return out


def record(refs, s, t, ratio):
    """(good_count, min_dist, n_train) of frame s against stored frame t"""
    knn = refs[(s, t)]                              # (no side is empty: the first two arguments only say so)
    good, dmin = ratioref.ratio_counts(knn[0], knn[0], ratio, knn)
    return good, dmin, K.ROWS[t]


def as_records(pkg, triples):
    a = np.zeros(len(triples), pkg.capi.SCORE_DTYPE)
    for k, tr in enumerate(triples):
        a[k] = tr
    return a


def as_list(rows, tidx, dist):
    out = np.zeros(len(rows), [(f, "<i4") for f in FIELDS[:3]] + [("distance", "<f4")])
    out["query_idx"], out["train_idx"], out["distance"] = rows, tidx, dist
    return out


def assert_same_list(got, want, msg=""):
    assert len(got) == len(want), (msg, len(got), len(want))
    for f in FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{msg} {f}")


def assert_records(got, want, msg=""):
    assert len(got) == len(want), (msg, len(got), len(want))
    for f in ("good_count", "min_dist", "n_train"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{msg} {f}")


def as_cands(pkg, want):
    a = np.zeros(len(want), pkg.capi.CANDIDATE_DTYPE)
    for k, (cur, matched, good, sim) in enumerate(want):
        a[k] = (cur, matched, good, 0, sim)
    return a


def bulk_ratio(m, pkg, ratio, **query_set):
    """(records, offsets) of one all_vs_all_ratio call; the device buffer is poisoned first."""
    n, offs = m.all_vs_all_ratio_plan(ratio, **query_set)
    got = np.zeros(n, pkg.capi.SCORE_DTYPE)
    if n:
        d = m.dev_alloc(n * 8)
        try:
            m.dev_upload(d, np.full(n * 8, 0xAB, np.uint8))
            assert m.all_vs_all_ratio(ratio, d, n, **query_set) == n
            m.sync()
            m.dev_download(d, got)
        finally:
            m.dev_free(d)
    return got, offs


@pytest.fixture(scope="module")
def tm(pkg, tall):
    """This module's own matcher holding the tall set, min_gap = 5."""
    p = pkg.default_params()
    p.min_gap = K.GAP
    m = pkg.Matcher(p)
    try:
        m.reserve(len(K.ORDER), 65535)
        for fid, rows in tall.stored():
            m.append(fid, rows)
        yield m
    finally:
        m.close()


def test_the_set_is_stored_with_its_hostile_rows(tm, tall):
    assert len(tm) == 6
    for slot, n in enumerate(K.ORDER):
        assert tm.frame_info(slot)[:2] == (K.IDS[n], K.ROWS[n])
        np.testing.assert_array_equal(tm.read_frame(slot), tall.frames[n])
    for t in K.TALL:                                # behind each tall frame: copies of its last row in rows 0 and 1 of the next slot
        nxt = tm.read_frame(K.ORDER.index(K.NEXT[t]))
        assert (nxt[:2] == tall.frames[t][-1]).all()


# ---- pair mode, stored -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ratio", RATIOS)
def test_stored_ratio_lists_against_tall_frames(tm, tall, refs, ratio):
    """lcm_match_stored_ratio, lcm_match_stored_batch_ratio and lcm_match_query_batch_ratio: X against A, Y and Z against
    A, B and C.  A padding copy or a next-slot row taken for a neighbour empties the trapped rows' part of Y's lists."""
    m, ids = tm, K.IDS
    want = {pr: as_list(*knnref.ratio_filter(*refs[pr], ratio)) for pr in STORED_PAIRS}
    for t in K.TALL:
        w = want[("Y", t)]
        trapped = w[np.isin(w["query_idx"], list(K.TRAP_ROWS[t]))]
        assert len(trapped) == 64 and (trapped["train_idx"] == K.ROWS[t] - 1).all() and (trapped["distance"] == 0).all()
    for s, t in STORED_PAIRS:
        assert_same_list(m.match_stored_ratio(ids[s], ids[t], ratio), want[(s, t)], f"stored {s} x {t} at {ratio}")
    lists, offs = m.match_stored_batch_ratio([(ids[s], ids[t]) for s, t in STORED_PAIRS], ratio)
    for pr, got in zip(STORED_PAIRS, lists):
        assert_same_list(got, want[pr], f"stored batch {pr} at {ratio}")
    assert offs.tolist() == np.cumsum([0] + [len(want[pr]) for pr in STORED_PAIRS]).tolist()
    for s in K.SMALL:
        trains = [t for t in K.TALL if (s, t) in want]
        lists, offs = m.match_query_batch_ratio(tall.frames[s], [ids[t] for t in trains], ratio)
        for t, got in zip(trains, lists):
            assert_same_list(got, want[(s, t)], f"query batch {s} x {t} at {ratio}")
        assert offs.tolist() == np.cumsum([0] + [len(want[(s, t)]) for t in trains]).tolist()


def test_tall_x_tall_stored_list(tm, tall, refs):
    """A (65535 query rows: 32 chunks of 2048) against stored B through lcm_match_stored_ratio at 1.0, and the same rows as
    the host query of lcm_match_query_batch_ratio: the planted rows and 512 sampled query rows in full against the numpy
    scan; for every row of the list the train index in range, the distance recomputed, query_idx strictly ascending."""
    A, B = tall.frames["A"], tall.frames["B"]
    sample, (ri, rd) = refs["sample"], refs["AxB"]
    rows, tidx, dist = knnref.ratio_filter(ri, rd, 1.0)
    want = as_list(sample[rows], tidx, dist)
    assert len(want) > 400                          # random rows: best < second almost always
    at = {int(q): k for k, q in enumerate(sample)}
    for f in tall.tall_found:                      # the reference finds what was planted
        k = at[f.qr]
        assert (int(ri[k, 0]), int(rd[k, 0]), int(ri[k, 1]), int(rd[k, 1])) == (f.i1, f.d1, f.i2, f.d2), f

    def check(lst, msg):
        assert 0 < len(lst) <= 65535 and not lst["img_idx"].any(), msg
        assert np.all(np.diff(lst["query_idx"]) > 0) and lst["query_idx"].min() >= 0 and lst["query_idx"].max() < 65535, msg
        assert lst["train_idx"].min() >= 0 and lst["train_idx"].max() < 65534, msg
        d = np.bitwise_count(A[lst["query_idx"]].view(np.uint64) ^ B[lst["train_idx"]].view(np.uint64)).sum(axis=1)
        np.testing.assert_array_equal(d, lst["distance"].astype(np.int64), err_msg=msg)
        assert_same_list(lst[np.isin(lst["query_idx"], sample)], want, f"{msg}: planted and sampled rows")
        for f in tall.tall_found:                  # (b) rows fail the strict test
            assert (f.qr in lst["query_idx"]) == (f.d1 < f.d2), (msg, f)

    check(tm.match_stored_ratio(K.IDS["A"], K.IDS["B"], 1.0, cap=65536), "stored A x B")
    lists, offs = tm.match_query_batch_ratio(A, [K.IDS["B"]], 1.0)
    assert offs.tolist() == [0, len(lists[0])]
    check(lists[0], "host A x stored B")


# ---- pair mode, host ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nt", [33, 513])
def test_knn2_pair_with_65535_query_rows(pkg, refs, nt):
    """65535 x 33 (one train segment, 128 query chunks) and 65535 x 513 from the host: every row, both neighbours."""
    case = refs["cases"][nt]
    ri, rd = refs[nt]
    m = pkg.Matcher()
    try:
        idx, dist = m.knn2_pair(case.query, case.train)
        info = m.launch_info()
        assert info.distances == 65535 * nt
        np.testing.assert_array_equal(idx, ri)
        np.testing.assert_array_equal(dist, rd)
        assert idx.shape == (65535, 2) and idx.min() >= 0 and idx.max() < nt
        for f in case.found:
            assert (idx[f.qr].tolist(), dist[f.qr].tolist()) == ([f.i1, f.i2], [f.d1, f.d2]), f
        i1, d1 = m.match_pair(case.query, case.train)            # second witness: the k = 1 call on neighbour 0
        np.testing.assert_array_equal(idx[:, 0], i1)
        np.testing.assert_array_equal(dist[:, 0], d1)
        want = as_list(*knnref.ratio_filter(ri, rd, 0.7))
        assert_same_list(m.match_features_ratio(case.query, case.train, 0.7), want, f"65535 x {nt}")
    finally:
        m.close()


@pytest.fixture(scope="module")
def wide():
    case = K.wide2_case()
    idx, dist = K.wide2_scan(case)
    K.check_wide2_scan(case, idx, dist)             # the scan finds what was planted
    return case, idx, dist


def test_knn2_pair_with_2_22_train_rows(pkg, wide):
    """lcm_knn2_pair / lcm_match_features_ratio on the wide case: 40 rows (above 64 M distances: the throughput shape,
    k_knn2_rowlane<64, 8>) and the first 16 (the latency shape, <256, 2>) under LCM_TUNE_PAIR_UPLOAD_KERNEL x
    LCM_TUNE_PAIR_HOST_FOLD: both neighbours of every row equal the numpy scan — segment-local keys plus g * seg_rows up
    to row 2^22 - 1, one below the distance field, and the host's 22-bit decode of BOTH keys."""
    cp = pkg.capi
    case, w_idx, w_dist = wide
    m = pkg.Matcher()
    try:
        for nq in (len(case.query), 16):
            for up in (1, 0):
                for fold in (1, 0):
                    m.set_tuning(cp.TUNE_PAIR_UPLOAD_KERNEL, up)
                    m.set_tuning(cp.TUNE_PAIR_HOST_FOLD, fold)
                    label = f"nq {nq} upload kernel {up} host fold {fold}"
                    idx, dist = m.knn2_pair(case.query[:nq], case.train)
                    info = m.launch_info()
                    assert info.distances == nq * K.WIDE_NT and info.launches == 2
                    # one work item per train segment (one query chunk in either shape): ties pair_segment_rows to the product
                    assert info.workgroups == -(-K.WIDE_NT // K.WIDE_SEG), (info.workgroups, K.WIDE_SEG, label)
                    np.testing.assert_array_equal(idx, w_idx[:nq], err_msg=label)
                    np.testing.assert_array_equal(dist.astype(np.int32), w_dist[:nq], err_msg=label)
        m.set_tuning(cp.TUNE_PAIR_UPLOAD_KERNEL, 1)
        m.set_tuning(cp.TUNE_PAIR_HOST_FOLD, 1)
        i1, d1 = m.match_pair(case.query, case.train)                # second witness on neighbour 0
        np.testing.assert_array_equal(i1, w_idx[:, 0])
        np.testing.assert_array_equal(d1.astype(np.int32), w_dist[:, 0])
        sizes = []
        for ratio in (0.7, 1.0):
            want = as_list(*knnref.ratio_filter(w_idx, w_dist.astype(np.uint16), ratio))
            assert_same_list(m.match_features_ratio(case.query, case.train, ratio), want, f"wide at {ratio}")
            sizes.append(len(want))
        assert 0 < sizes[0] < sizes[1] < len(case.query) and int(want["train_idx"].max()) == K.WIDE_NT - 1
    finally:
        m.close()


# ---- ratio search ------------------------------------------------------------------------------------------------------

class ExternalSet:
    """query frames as a device-resident external query set"""

    def __init__(self, m, queries):
        self.m = m
        stride = max(len(r) for _, r in queries)
        rows = np.zeros((len(queries), stride, 32), np.uint8)
        for k, (_, r) in enumerate(queries):
            rows[k, : len(r)] = r
        counts = np.array([len(r) for _, r in queries], np.int32)
        self.d_rows, self.d_counts = m.dev_alloc(rows.nbytes), m.dev_alloc(counts.nbytes)
        m.dev_upload(self.d_rows, rows)
        m.dev_upload(self.d_counts, counts)
        self.kw = dict(d_query_rows=self.d_rows, d_query_counts=self.d_counts, q_ids=[i for i, _ in queries], q_stride_rows=stride)

    def free(self):
        self.m.dev_free(self.d_rows)
        self.m.dev_free(self.d_counts)


def loop_expect(refs, ratio, min_rows, min_matches, small=K.SMALL, ids=None):
    """the reference's rule (ratioloopref.verdict) over the eligible (small, tall) pairs, in (current, matched) order"""
    out = []
    for s in small:
        for t in K.TALL:
            good = record(refs, s, t, ratio)[0]
            if all(R.verdict(good, K.ROWS[s], K.ROWS[t], min_rows, min_matches)):
                out.append(((ids or K.IDS)[s], K.IDS[t], good, R.similarity(good, K.ROWS[s], K.ROWS[t])))
    return out


def test_ratio_search_against_tall_stored_frames(pkg, tm, tall, refs):
    """lcm_all_vs_all_ratio self (9 pairs: frames 0 .. 2 have no eligible partner and, being no query frames, do not make
    the call refuse their 65535 rows) and from an external query set, lcm_query_scores_ratio, lcm_detect_loops_ratio host
    and stored: every record in every field, n_train 65535 / 65534 / 65533 (bit 15 of the record's field)."""
    m, fr = tm, tall.frames
    for ratio in (0.7, 1.0):
        want = as_records(pkg, [record(refs, s, t, ratio) for s, t in ALL_PAIRS])
        got, offs = bulk_ratio(m, pkg, ratio)
        assert offs.tolist() == [0, 0, 0, 0, 3, 6, 9]
        assert_records(got, want, f"self at {ratio}")
        assert got["n_train"].tolist() == [65535, 65534, 65533] * 3
        info = m.launch_info()
        assert (info.route, info.launches, info.pairs) == (pkg.capi.ROUTE_PLAIN, 1, 9)
        assert info.distances == sum(K.ROWS[s] * K.ROWS[t] for s, t in ALL_PAIRS)
        # the trap: 64 rows of Y at distance 0 from each tall frame's last row count (a copy as second neighbour: none does)
        for k, (s, t) in enumerate(ALL_PAIRS):
            if s == "Y":
                assert got[k]["good_count"] >= 64 and got[k]["min_dist"] == 0
        ext = ExternalSet(m, [(7 + k, fr[s]) for k, s in enumerate(K.SMALL)])      # ids 7, 8, 9: A, B and C eligible, no more
        try:
            e_got, e_offs = bulk_ratio(m, pkg, ratio, **ext.kw)
            assert e_offs.tolist() == [0, 3, 6, 9]
            assert_records(e_got, want, f"external at {ratio}")
            ext.kw["q_ids"] = [100, 101, 102]                                      # far ids: the small frames are eligible too
            e_got, e_offs = bulk_ratio(m, pkg, ratio, **ext.kw)
            far = as_records(pkg, [record(refs, s, t, ratio) for s in K.SMALL for t in K.ORDER])
            assert e_offs.tolist() == [0, 6, 12, 18]
            assert_records(e_got, far, f"external, far ids, at {ratio}")
        finally:
            ext.free()
        for k, s in enumerate(K.SMALL):
            sc, ids = m.query_scores_ratio(fr[s], K.IDS[s], ratio)
            assert ids.tolist() == [0, 1, 2]
            assert_records(sc, want[3 * k: 3 * k + 3], f"online {s} at {ratio}")
    # the loop rule over those records: host rows and the stored frame; min_matches at Y x A's count and one above
    c_ya = record(refs, "Y", "A", 0.7)[0]
    for rp in ((0.7, 96, 1), (0.7, 97, 1), (0.7, 513, c_ya), (0.7, 513, c_ya + 1), (0.7, 0, 0), (1.0, 514, 100)):
        for s in K.SMALL:
            w = as_cands(pkg, loop_expect(refs, *rp, small=(s,)))
            assert m.detect_loops_ratio(K.IDS[s], fr[s], *rp).tobytes() == w.tobytes(), (rp, s, "host rows")
            assert m.detect_loops_ratio(K.IDS[s], None, *rp).tobytes() == w.tobytes(), (rp, s, "stored")
    assert (K.IDS["Y"], K.IDS["A"]) in [(c, t) for c, t, _, _ in loop_expect(refs, 0.7, 513, c_ya)]
    assert (K.IDS["Y"], K.IDS["A"]) not in [(c, t) for c, t, _, _ in loop_expect(refs, 0.7, 513, c_ya + 1)]


def test_fused_loop_search_and_group_on_the_tall_set(pkg, tm, tall, refs, tmp_path):
    """lcm_all_vs_all_loops_ratio: min_rows 65533 .. 65536 (a bound that only A, B, C could meet: the rule asks it of BOTH
    frames, and a query frame has at most 2048 rows here, so the expected list is empty — as the host rule says), min_rows
    around the small frames' own 96 / 513 / 2048 rows, min_matches at the trap pair's count and one above; the score array
    it leaves == a separate lcm_all_vs_all_ratio download; one W = 3 loopback group loaded with the set returns the single
    handle's bytes."""
    m = tm
    c_ya = record(refs, "Y", "A", 0.7)[0]
    sep, _ = bulk_ratio(m, pkg, 0.7)
    rps = [(0.7, r, 1) for r in (65533, 65534, 65535, 65536, 96, 97, 513, 514, 2048, 2049)]
    rps += [(0.7, 0, c_ya), (0.7, 0, c_ya + 1), (0.7, 0, 0), (1.0, 96, 200)]
    single = {}
    for rp in rps:
        got, n_pairs = m.all_vs_all_loops_ratio(*rp)
        want = loop_expect(refs, *rp)
        assert n_pairs == 9
        assert got.tobytes() == as_cands(pkg, want).tobytes(), (rp, got, want)
        if rp[0] == 0.7:
            left = m.last_bulk_scores()
            assert left.tobytes() == sep.tobytes(), rp
            assert left["n_train"].tolist() == [65535, 65534, 65533] * 3
        single[rp] = got.copy()
    assert len(single[(0.7, 65533, 1)]) == 0 and len(single[(0.7, 96, 1)]) == 9 and len(single[(0.7, 97, 1)]) == 6
    assert len(single[(0.7, 0, c_ya)]) == len(single[(0.7, 0, c_ya + 1)]) + sum(record(refs, s, t, 0.7)[0] == c_ya for s, t in ALL_PAIRS)
    path = str(tmp_path / "tall2.lcmdb")
    m.save(path)
    p = pkg.default_params()
    p.min_gap = K.GAP
    with pkg.Group(p, n_devices=3, loopback_device=0) as g:
        g.load(path)
        assert len(g) == 6 and g.world == 3
        got, offs = g.all_vs_all_ratio(0.7)
        assert got.tobytes() == sep.tobytes() and offs.tolist() == [0, 0, 0, 0, 3, 6, 9]
        for rp in ((0.7, 96, 1), (0.7, 0, c_ya), (0.7, 65535, 1)):
            gc, n_pairs = g.all_vs_all_loops_ratio(*rp)
            assert n_pairs == 9 and gc.tobytes() == single[rp].tobytes(), rp


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_and_its_results_unchanged(pkg, tm, tall, wide):
    """LCM_ERR_CAPACITY, each decided before anything is launched: all_vs_all_ratio_impl refuses while it builds the plan
    (max_q_rows, before wait_db and the launch loop), query_scores_ratio_impl on its nq argument before set_device,
    run_pair_jobs on jb.nt in its planning loop before the staging block is sized."""
    cp, m, fr = pkg.capi, tm, tall.frames
    before, _ = bulk_ratio(m, pkg, 0.7)

    def refused(fn, *a, **kw):
        with pytest.raises(cp.LcmError) as e:
            fn(*a, **kw)
        assert e.value.code == cp.ERR_CAPACITY, e.value
        assert len(str(e.value)) > 20                       # says why

    d = m.dev_alloc(64 * 8)
    try:
        m.set_params(min_gap=1)                             # a tall frame becomes a query frame
        try:
            refused(m.all_vs_all_ratio_plan, 0.7)
            refused(m.all_vs_all_ratio, 0.7, d, 64)
            refused(m.all_vs_all_loops_ratio, 0.7, 0, 0)
            refused(m.detect_loops_ratio, K.IDS["B"], None, 0.7, 0, 0)       # a stored 65534-row frame as the query
        finally:
            m.set_params(min_gap=K.GAP)
        too_tall = np.zeros((65536, 32), np.uint8)
        for q in (tall.refused, too_tall, fr["C"]):
            refused(m.query_scores_ratio, q, 50, 0.7)
            refused(m.detect_loops_ratio, 50, q, 0.7, 0, 0)
        ext = ExternalSet(m, [(50, tall.refused)])
        try:
            refused(m.all_vs_all_ratio_plan, 0.7, **ext.kw)
        finally:
            ext.free()
        train = np.concatenate([wide[0].train, wide[0].train[:1]])
        assert len(train) == K.WIDE_NT + 1
        refused(m.knn2_pair, fr["Z"], train)
        refused(m.match_query_batch_ratio, np.zeros((131073, 32), np.uint8), [K.IDS["A"]], 0.7)      # above 64 x 2048 query rows
        refused(m.match_features_ratio, fr["Z"], train, 0.7)
        idx, dist = m.knn2_pair(fr["Z"][:4], train[1:])      # 2^22 rows: served (row 0 went to the end)
        want = [K.scan2(train[1:], fr["Z"][r]) for r in range(4)]
        assert [[(int(i), int(x)) for i, x in zip(idx[r], dist[r])] for r in range(4)] == want
    finally:
        m.dev_free(d)
    after, _ = bulk_ratio(m, pkg, 0.7)
    assert after.tobytes() == before.tobytes() and len(m) == 6
    sc, ids = m.query_scores_ratio(fr["Z"], K.IDS["Z"], 0.7)
    assert sc.tobytes() == before[6:9].tobytes() and ids.tolist() == [0, 1, 2]


# ---- online call: stored slots per workgroup -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def table():
    return K.table_set()


def query70(table):
    """70 query rows: every type's rows, twice over, and random rows"""
    rng = np.random.default_rng(70)
    rows = np.concatenate([t for t in table.types] * 2 + [K.rnd(rng, 8)])
    assert len(rows) == 70
    return rows


def test_online_ratio_call_slots_per_workgroup(pkg, table):
    """lcm_query_scores_ratio gives a workgroup 1 stored slot below 4096 eligible frames, 2 from 4096 and 4 from 8192, the
    last workgroup min(spi, n - slot_begin): 4095 .. 8200 eligible frames of 8 types by slot."""
    cp = pkg.capi
    q = query70(table)
    by_type = as_records(pkg, [ratioref.ratio_counts(q, t, 0.7) + (len(t),) for t in table.types])
    assert len(set(by_type["good_count"].tolist())) >= 5
    ty = K.type_of(np.arange(K.N_ONLINE))
    p = pkg.default_params()
    p.min_gap = 1
    m = pkg.Matcher(p)
    try:
        m.reserve(K.N_ONLINE, 9)
        for s, rows in table.frames(K.N_ONLINE):
            m.append(s, rows)
        for n, spi in ((4095, 1), (4096, 2), (4097, 2), (8191, 2), (8192, 4), (8193, 4), (8200, 4)):
            sc, ids = m.query_scores_ratio(q, n, 0.7)                # ids 0 .. n - 1 are eligible
            info = m.launch_info()
            assert (info.launches, info.pairs, info.workgroups) == (1, n, -(-n // spi)), (n, info.workgroups)
            assert_records(sc, by_type[ty[:n]], f"{n} eligible frames")
            _, plain_ids = m.query_scores(q, n)
            np.testing.assert_array_equal(ids, plain_ids)
            assert ids.tolist() == list(range(n))
    finally:
        m.close()


# ---- bulk call: more work items than one launch takes ----------------------------------------------------------------------

def test_bulk_ratio_search_in_two_launches(pkg, table):
    """1449 stored frames, one stored slot per work item: 1,049,076 items, 2^20 in the first launch and 500 in the second
    (a.items = P.d_items + first).  Every record == the type table; the fused loop search over them == the host rule."""
    cp = pkg.capi
    n = K.N_SLICE
    ty = K.type_of(np.arange(n))
    c, s = np.tril_indices(n, -1)                                  # (query ascending, stored ascending)
    assert len(c) == 1049076 > 1 << 20
    g7, m7 = table.table(0.7)
    rows = np.array(K.TYPE_ROWS)
    p = pkg.default_params()
    p.min_gap = 1
    m = pkg.Matcher(p)
    try:
        for slot, r in table.frames(n):
            m.append(slot, r)
        m.set_tuning(cp.TUNE_ITEM_SLOTS, 1)
        got, offs = bulk_ratio(m, pkg, 0.7)
        info = m.launch_info()
        assert (info.launches, info.workgroups, info.pairs) == (2, 1 << 20, len(c))
        assert offs.tolist() == [k * (k - 1) // 2 for k in range(n + 1)]
        np.testing.assert_array_equal(got["good_count"], g7[ty[c], ty[s]])
        np.testing.assert_array_equal(got["min_dist"], m7[ty[c], ty[s]])
        np.testing.assert_array_equal(got["n_train"], rows[ty[s]])
        min_matches = 7
        good = g7[ty[c], ty[s]].astype(np.int64)
        keep = good >= min_matches
        assert 0.01 < keep.mean() < 0.10
        cands, n_pairs = m.all_vs_all_loops_ratio(0.7, 0, min_matches)
        assert n_pairs == len(c) and len(cands) == int(keep.sum())
        np.testing.assert_array_equal(cands["current_frame_id"], c[keep])
        np.testing.assert_array_equal(cands["matched_frame_id"], s[keep])
        np.testing.assert_array_equal(cands["num_matches"], good[keep])
        den = np.minimum(rows[ty[c]], rows[ty[s]])[keep].astype(np.float64)
        assert cands["similarity_score"].tobytes() == (good[keep].astype(np.float64) / den).tobytes()
        assert m.last_bulk_scores().tobytes() == got.tobytes()
    finally:
        m.set_tuning(cp.TUNE_ITEM_SLOTS, 0)
        m.close()

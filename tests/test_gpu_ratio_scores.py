"""lcm_all_vs_all_ratio / lcm_query_scores_ratio on the device against tests/ratioref.py: the reference's loop-search score
(src/main.cpp:1375-1388: the number of survivors of knnMatch(k = 2) + Lowe's ratio test per pair), exact in every field of
every record.  Needs a real MI355X."""
import numpy as np
import pytest

import knnref
import ratioref

pytestmark = pytest.mark.gpu

RATIOS = (0.5, 0.7, 0.75, 0.8, 1.0, 1.5)
EMPTY = np.zeros((0, 32), np.uint8)


def rnd(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip(rng, row, k):
    """`row` with exactly k of its 256 bits flipped."""
    m = np.zeros(256, np.uint8)
    m[rng.choice(256, int(k), replace=False)] = 1
    return row ^ np.packbits(m, bitorder="little")


@pytest.fixture
def db(matcher, pkg):
    """The session's matcher, emptied, with min_gap = 1; parameters and tuning knobs are put back afterwards."""
    before = matcher.params
    matcher.clear()
    matcher.set_params(min_gap=1)
    yield matcher
    matcher.set_tuning(pkg.capi.TUNE_ITEM_SLOTS, 0)
    matcher.set_tuning(pkg.capi.TUNE_PACKED, -1)
    matcher.set_params(**{f: getattr(before, f) for f, _ in pkg.capi.Params._fields_})
    matcher.clear()


def fill(m, frames):
    for fid, rows in frames:
        m.append(int(fid), rows)


class Ref:
    """Expected records of a list of (id, rows) frames used as database and query set; knnMatch(k = 2) of a pair is
    computed once and shared by every ratio."""

    def __init__(self, frames):
        self.frames = frames
        self.knn = {}

    def pair(self, c, s, ratio):
        q, t = self.frames[c][1], self.frames[s][1]
        if len(q) and len(t) and (c, s) not in self.knn:
            self.knn[(c, s)] = knnref.knn2(q, t)
        good, dmin = ratioref.ratio_counts(q, t, ratio, self.knn.get((c, s)))
        return good, dmin, len(t)

    def eligible(self, query_id, gap):
        return [s for s, (fid, _) in enumerate(self.frames) if query_id - fid >= max(gap, 1)]

    def records(self, ratio, gap=1, queries=None):
        """(records in (query ascending, stored ascending) order, offsets[n_queries + 1])"""
        out, offs = [], [0]
        for c in (range(len(self.frames)) if queries is None else queries):
            out += [self.pair(c, s, ratio) for s in self.eligible(self.frames[c][0], gap)]
            offs.append(len(out))
        return out, offs


def as_records(pkg, triples):
    a = np.zeros(len(triples), pkg.capi.SCORE_DTYPE)
    for k, (good, dmin, nt) in enumerate(triples):
        a[k] = (good, dmin, nt)
    return a


def bulk_ratio(m, pkg, ratio, **query_set):
    """(records, offsets) of one all_vs_all_ratio call; the device buffer is poisoned first."""
    n, offs = m.all_vs_all_ratio_plan(ratio, **query_set)
    got = np.zeros(n, pkg.capi.SCORE_DTYPE)
    if n:
        d = m.dev_alloc(n * 8)
        m.dev_upload(d, np.full(n * 8, 0xAB, np.uint8))
        assert m.all_vs_all_ratio(ratio, d, n, **query_set) == n
        m.sync()
        m.dev_download(d, got)
        m.dev_free(d)
    return got, offs


def assert_records(got, want, msg=""):
    assert len(got) == len(want), (msg, len(got), len(want))
    for f in ("good_count", "min_dist", "n_train"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{msg} {f}")


def check_bulk(m, pkg, ref, ratio, gap=1, msg=""):
    got, offs = bulk_ratio(m, pkg, ratio)
    want, woffs = ref.records(ratio, gap)
    assert offs.tolist() == woffs, msg
    assert_records(got, as_records(pkg, want), f"{msg} ratio {ratio}")
    return got, offs


# ---- padding rows and the second neighbour ---------------------------------------------------------------------------

NT_EDGES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 33, 65)


def test_padding_rows_never_become_the_second_neighbour(db, pkg):
    """Stored frames are padded to a multiple of 4 rows with copies of their last row.  70 query rows equal to x against
    (a) nt identical rows: second == best, nothing survives a ratio <= 1; (b) the LAST row equal to x and the others
    253 bits or more away: all 70 survive at 0.7 — unless a padding copy of the last row is taken for the second."""
    rng = np.random.default_rng(700)
    x = rnd(rng, 1)
    frames, same, trap = [], [], []
    for nt in NT_EDGES:
        same.append(len(frames))
        frames.append((len(frames), np.repeat(rnd(rng, 1), nt, axis=0)))
        t = np.repeat(~x, nt, axis=0)
        for r in range(nt - 1):
            t[r, rng.integers(0, 32, 3)] ^= np.uint8(1 << int(rng.integers(0, 8)))
        t[nt - 1] = x
        trap.append(len(frames))
        frames.append((len(frames), t))
    qf = len(frames)
    frames.append((qf, np.repeat(x, 70, axis=0)))
    fill(db, frames)
    ref = Ref(frames)
    for ratio in (0.7, 1.0):
        got, offs = check_bulk(db, pkg, ref, ratio)
        mine = got[int(offs[qf]): int(offs[qf + 1])]          # the 70-row frame against every stored frame
        assert len(mine) == qf
        for nt, s in zip(NT_EDGES, same):
            assert mine[s]["good_count"] == 0 and mine[s]["n_train"] == nt
        for nt, s in zip(NT_EDGES, trap):
            assert mine[s]["min_dist"] == 0
            assert mine[s]["good_count"] == (0 if nt == 1 else 70), (ratio, nt)


# ---- a run of stored slots inside one work item ----------------------------------------------------------------------

@pytest.mark.parametrize("item_slots", [1, 2, 0, 8])
def test_slot_run_inside_one_item(db, pkg, place, item_slots):
    """Five eligible stored frames of 1, 4, 0, 5 and 9 rows: the running distances are reset per slot, the empty frame
    gets its empty record, and the per-pair reduction words alternate correctly across consecutive slots."""
    rng = np.random.default_rng(710)
    base = place.frames[0][1]
    frames = [(i, np.stack([flip(rng, base[int(rng.integers(0, 40))], int(rng.integers(0, 50))) for _ in range(n)]) if n else EMPTY)
              for i, n in enumerate((1, 4, 0, 5, 9))]
    frames.append((5, base[:70]))
    db.set_tuning(pkg.capi.TUNE_ITEM_SLOTS, item_slots)
    fill(db, frames)
    ref = Ref(frames)
    for ratio in (0.7, 1.0):
        got, offs = check_bulk(db, pkg, ref, ratio, msg=f"item_slots {item_slots}")
        last = got[int(offs[5]):]
        assert last["n_train"].tolist() == [1, 4, 0, 5, 9]
        assert tuple(last[2]) == (0, 0xFFFF, 0) and last[0]["good_count"] == 0
    assert sum(int(g) for g in last["good_count"]) > 0


# ---- workgroup shapes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq", [1, 63, 64, 65, 257, 512, 513, 1025, 1537, 2048])
def test_workgroup_shapes(db, pkg, nq):
    """64 / 128 / 192 / 256-thread workgroups of 8 rows per lane, a lane's 8 rows partly valid; bulk and online call."""
    rng = np.random.default_rng(720 + nq)
    t0, t1 = rnd(rng, 37), rnd(rng, 64)
    q = rnd(rng, nq)
    for r in range(0, nq, 3):                     # near-duplicates of stored rows, some of them twice in the stored frame
        q[r] = flip(rng, t0[r % 37], int(rng.integers(0, 60)))
    t0[36] = t0[5]; t1[63] = t0[7]; t1[10] = flip(rng, t0[7], 9)
    frames = [(0, t0), (1, t1), (2, q)]
    fill(db, frames)
    ref = Ref(frames)
    got, offs = check_bulk(db, pkg, ref, 0.7, msg=f"nq {nq}")
    assert db.launch_info().route == pkg.capi.ROUTE_PLAIN
    scores, ids = db.query_scores_ratio(q, 2, 0.7)
    assert ids.tolist() == [0, 1]
    assert_records(scores, got[int(offs[2]):], f"online nq {nq}")


# ---- ratios ----------------------------------------------------------------------------------------------------------

class Place:
    pass


@pytest.fixture(scope="module")
def place():
    """Six frames of one place (~150 rows each): per base row a frame holds no copy, one noisy copy, two noisy copies or
    two EXACT copies (second == best == 0: fails every ratio), plus unrelated rows; frame 0 / frame 5 also carry, per
    tested ratio, a row planted exactly on the boundary (d1 < ratio * d2, d1 + 1 not)."""
    rng = np.random.default_rng(730)
    base = rnd(rng, 96)
    frames = []
    for f in range(6):
        rows = []
        for b in base:
            u = rng.random()
            if u < 0.10:
                rows += [b, b]
            elif u < 0.40:
                rows.append(flip(rng, b, rng.integers(0, 30)))
            elif u < 0.75:
                rows += [flip(rng, b, rng.integers(0, 30)), flip(rng, b, rng.integers(15, 60))]
        rows += list(rnd(rng, 40))
        rows = np.stack(rows)[rng.permutation(len(rows))]
        frames.append([f, rows])
    # boundary rows: query row y (frame 5), stored rows y ^ (d1 bits) and y ^ (d2 bits) (frame 0) with d1 <= d2 <= 40,
    # d1 = lim[d2] - 1: the largest d1 that passes against that d2
    extra_q, extra_t = [], []
    for ratio in RATIOS:
        lim = ratioref.lim_table(ratio)
        d1, d2 = next((int(lim[d]) - 1, d) for d in range(40, 0, -1) if 0 <= int(lim[d]) - 1 <= d)
        y = rnd(rng, 1)[0]
        extra_q.append(y)
        extra_t += [flip(rng, y, d1), flip(rng, y, d2)]
    frames[5][1] = np.concatenate([frames[5][1], np.stack(extra_q)])
    frames[0][1] = np.concatenate([frames[0][1], np.stack(extra_t)])
    p = Place()
    p.frames = [(f, rows) for f, rows in frames]
    p.ref = Ref(p.frames)
    p.want = {ratio: p.ref.records(ratio) for ratio in RATIOS}
    return p


def test_ratios_select(place):
    """The inputs are not trivial (checked on the reference alone)."""
    for ratio in RATIOS:
        recs, offs = place.want[ratio]
        assert len(recs) == 15
        pairs = [(c, s) for c in range(6) for s in range(c)]
        partial = sum(0 < good < len(place.frames[c][1]) for (good, _, _), (c, _) in zip(recs, pairs))
        assert 2 * partial > len(recs), (ratio, partial)
        idx, dist = place.ref.knn[(5, 0)]
        d1, d2 = dist[:, 0].astype(np.float64), dist[:, 1].astype(np.float64)
        assert ((d1 < ratio * d2) & ~(d1 + 1 < ratio * d2)).any(), ratio
    goods = [sum(g for g, _, _ in place.want[ratio][0]) for ratio in RATIOS]
    assert goods == sorted(goods) and goods[0] < goods[-1]


@pytest.mark.parametrize("ratio", RATIOS)
def test_ratios(db, pkg, place, ratio):
    fill(db, place.frames)
    got, offs = bulk_ratio(db, pkg, ratio)
    want, woffs = place.want[ratio]
    assert offs.tolist() == woffs
    assert_records(got, as_records(pkg, want), f"ratio {ratio}")
    info = db.launch_info()
    assert (info.route, info.launches, info.pairs) == (pkg.capi.ROUTE_PLAIN, 1, 15)
    assert info.distances == sum(len(place.frames[c][1]) * len(place.frames[s][1]) for c in range(6) for s in range(c))
    assert info.kernel_ms > 0


def test_other_parameters_are_ignored(db, pkg, place):
    fill(db, place.frames)
    db.set_params(ratio=7, dist_floor=99, min_matches=1, sim_threshold=0.9)
    db.set_kernel_variant(1)
    try:
        got, _ = bulk_ratio(db, pkg, 0.75)
    finally:
        db.set_kernel_variant(0)
    assert_records(got, as_records(pkg, place.want[0.75][0]), "params")


# ---- min_gap, external query set -------------------------------------------------------------------------------------

def test_min_gap_and_external_query_set(db, pkg, place):
    ids = [0, 3, 4, 10, 11, 30]
    frames = [(i, rows) for i, (_, rows) in zip(ids, place.frames)]
    fill(db, frames)
    db.set_params(min_gap=5)
    ref = Ref(frames)
    ref.knn = place.ref.knn                        # same rows, same pair indices
    n_plain, offs_plain = db.all_vs_all_plan()
    got, offs = bulk_ratio(db, pkg, 0.7)
    want, woffs = ref.records(0.7, gap=5)
    assert offs.tolist() == offs_plain.tolist() == woffs and len(got) == n_plain
    assert woffs == [0, 0, 0, 0, 3, 6, 11]         # eligible prefixes 0, 0, 0, 3, 3, 5 of ids 0, 3, 4, 10, 11, 30
    assert_records(got, as_records(pkg, want), "min_gap 5")
    # the same frames as an external device query set
    stride = max(len(rows) for _, rows in frames)
    rows = np.zeros((len(frames), stride, 32), np.uint8)
    for k, (_, r) in enumerate(frames):
        rows[k, : len(r)] = r
    counts = np.array([len(r) for _, r in frames], np.int32)
    d_rows, d_counts = db.dev_alloc(rows.nbytes), db.dev_alloc(counts.nbytes)
    try:
        db.dev_upload(d_rows, rows)
        db.dev_upload(d_counts, counts)
        ext, eoffs = bulk_ratio(db, pkg, 0.7, d_query_rows=d_rows, d_query_counts=d_counts, q_ids=ids, q_stride_rows=stride)
        assert eoffs.tolist() == woffs
        assert_records(ext, got, "external query set")
        # and with ids of its own: every stored frame is eligible for every query frame
        far = [100 + i for i in range(len(frames))]
        ext, eoffs = bulk_ratio(db, pkg, 0.7, d_query_rows=d_rows, d_query_counts=d_counts, q_ids=far, q_stride_rows=stride)
        assert eoffs.tolist() == [6 * c for c in range(7)]
        for c in (1, 4):
            w = [ref.pair(c, s, 0.7) for s in range(6) if s != c]
            g = np.delete(ext[6 * c: 6 * c + 6], c)
            assert_records(g, as_records(pkg, w), f"external, own ids, query {c}")
    finally:
        db.dev_free(d_rows)
        db.dev_free(d_counts)


# ---- the online call -------------------------------------------------------------------------------------------------

def test_query_scores_ratio(db, pkg, place):
    fill(db, place.frames[:5])
    q = place.frames[5][1]
    plain_scores, plain_ids = db.query_scores(q, 5)
    for ratio in (0.7, 1.0):
        scores, ids = db.query_scores_ratio(q, 5, ratio)
        assert ids.tolist() == plain_ids.tolist() == [0, 1, 2, 3, 4]
        assert_records(scores, as_records(pkg, place.want[ratio][0][10:]), f"online {ratio}")
    info = db.launch_info()
    assert (info.route, info.launches, info.workgroups, info.pairs) == (pkg.capi.ROUTE_PLAIN, 1, 5, 5)
    # an outstanding ticket stays collectable, with unchanged records
    t = db.query_submit(q, 5)
    scores, _ = db.query_scores_ratio(q, 5, 0.7)
    s2, i2 = db.query_collect(t)
    np.testing.assert_array_equal(s2, plain_scores)
    np.testing.assert_array_equal(i2, plain_ids)
    assert_records(scores, as_records(pkg, place.want[0.7][0][10:]), "beside a ticket")
    # nothing eligible, and an empty query frame
    scores, ids = db.query_scores_ratio(q, 0, 0.7)
    assert len(scores) == 0 and len(ids) == 0
    scores, ids = db.query_scores_ratio(EMPTY, 5, 0.7)
    assert scores["good_count"].tolist() == [0] * 5 and scores["min_dist"].tolist() == [0xFFFF] * 5
    assert scores["n_train"].tolist() == [len(r) for _, r in place.frames[:5]]
    # appends issued just before the call are part of its answer
    db.append(5, q)
    scores, ids = db.query_scores_ratio(place.frames[0][1], 9, 1.0)
    assert ids.tolist() == [0, 1, 2, 3, 4, 5]
    assert tuple(scores[5]) == place.ref.pair(0, 5, 1.0)


# ---- against the pair mode's lists ------------------------------------------------------------------------------------

def test_counts_equal_the_pair_mode_list_lengths(db, pkg, place):
    fill(db, place.frames)
    got, offs = bulk_ratio(db, pkg, 0.7)
    pairs = [(5, 0), (5, 4), (3, 1), (1, 0), (4, 2), (2, 1)]
    lists, _ = db.match_stored_batch_ratio(pairs, 0.7)
    for (c, s), lst in zip(pairs, lists):
        assert got[int(offs[c]) + s]["good_count"] == len(lst), (c, s)


# ---- beside lcm_all_vs_all on one handle -------------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [-1, 1])
def test_alternates_with_all_vs_all(db, pkg, place, packed):
    fill(db, place.frames)
    db.set_tuning(pkg.capi.TUNE_PACKED, packed)

    def plain():
        n, _ = db.all_vs_all_plan()
        d = db.dev_alloc(n * 8)
        out = np.zeros(n, pkg.capi.SCORE_DTYPE)
        db.all_vs_all(d, n)
        route = db.launch_info().route
        db.sync()
        db.dev_download(d, out)
        db.dev_free(d)
        return out.tobytes(), route

    first, route = plain()
    assert route == (pkg.capi.ROUTE_PACKED if packed == 1 else pkg.capi.ROUTE_PLAIN)
    got, _ = bulk_ratio(db, pkg, 0.7)
    third, route3 = plain()
    assert first == third and route3 == route
    assert_records(got, as_records(pkg, place.want[0.7][0]), f"packed {packed}")
    again, _ = bulk_ratio(db, pkg, 0.7)
    assert again.tobytes() == got.tobytes()


# ---- errors ------------------------------------------------------------------------------------------------------------

def test_errors(db, pkg):
    m, E = db, pkg.capi
    rng = np.random.default_rng(750)
    q, t = rnd(rng, 20), rnd(rng, 30)
    fill(m, [(0, t), (1, q)])

    def code(fn, *a, **kw):
        with pytest.raises(pkg.LcmError) as e:
            fn(*a, **kw)
        return e.value.code

    d = m.dev_alloc(64)
    try:
        for bad in (float("nan"), -1.0):
            assert code(m.all_vs_all_ratio, bad, d, 8) == E.ERR_INVALID_ARG
            assert code(m.all_vs_all_ratio_plan, bad) == E.ERR_INVALID_ARG
            assert code(m.query_scores_ratio, q, 1, bad) == E.ERR_INVALID_ARG
        m.set_params(cross_check=1)
        try:
            assert code(m.all_vs_all_ratio, 0.7, d, 8) == E.ERR_INVALID_ARG
            assert code(m.query_scores_ratio, q, 1, 0.7) == E.ERR_INVALID_ARG
        finally:
            m.set_params(cross_check=0)
        # a too-small buffer: refused with nothing written
        m.dev_upload(d, np.full(64, 0xAB, np.uint8))
        assert m.all_vs_all_ratio_plan(0.7)[0] == 1
        assert code(m.all_vs_all_ratio, 0.7, d, 0) == E.ERR_CAPACITY
        back = np.zeros(64, np.uint8)
        m.sync()
        m.dev_download(d, back)
        assert (back == 0xAB).all()
        assert m.all_vs_all_ratio(0.7, d, 1) == 1
        # a query frame above 2048 rows
        big = rnd(rng, 2049)
        assert code(m.query_scores_ratio, big, 2, 0.7) == E.ERR_CAPACITY
        m.append(2, big)
        assert code(m.all_vs_all_ratio_plan, 0.7) == E.ERR_CAPACITY
        assert code(m.all_vs_all_ratio, 0.7, d, 8) == E.ERR_CAPACITY
        m.truncate(2)
        m.append(2, big[:2048])
        assert m.all_vs_all_ratio_plan(0.7)[0] == 3
    finally:
        m.dev_free(d)

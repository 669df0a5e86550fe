"""lcm_all_vs_all_loops_ratio / lcm_detect_loops_ratio on the device against tests/ratioloopref.py: the reference's loop
rule (src/main.cpp:1379-1388) on the ratio-test score, decided and compacted on the device.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import ratioloopref as R

pytestmark = pytest.mark.gpu


@pytest.fixture
def db(matcher, pkg):
    """The session's matcher, emptied, with min_gap = 1; parameters and tuning knobs are put back afterwards."""
    before = matcher.params
    matcher.clear()
    matcher.set_params(min_gap=1)
    yield matcher
    matcher.set_kernel_variant(0)
    matcher.set_params(**{f: getattr(before, f) for f, _ in pkg.capi.Params._fields_})
    matcher.clear()


def fill(m, frames):
    for fid, rows in frames:
        m.append(int(fid), rows)


def as_cands(pkg, want):
    a = np.zeros(len(want), pkg.capi.CANDIDATE_DTYPE)
    for k, (cur, matched, good, sim) in enumerate(want):
        a[k] = (cur, matched, good, 0, sim)
    return a


def assert_cands(pkg, got, want, msg=""):
    """field by field, similarity as float64 bits, order strictly ascending in (current, matched)"""
    w = as_cands(pkg, want)
    assert len(got) == len(w), (msg, len(got), len(w))
    for f in ("current_frame_id", "matched_frame_id", "num_matches"):
        np.testing.assert_array_equal(got[f], w[f], err_msg=f"{msg} {f}")
    assert got["similarity_score"].tobytes() == w["similarity_score"].tobytes(), msg
    keys = list(zip(got["current_frame_id"].tolist(), got["matched_frame_id"].tolist()))
    assert all(a < b for a, b in zip(keys, keys[1:])), msg


def ratio_scores(m, pkg, ratio, **query_set):
    n, _ = m.all_vs_all_ratio_plan(ratio, **query_set)
    got = np.zeros(n, pkg.capi.SCORE_DTYPE)
    if n:
        d = m.dev_alloc(n * 8)
        assert m.all_vs_all_ratio(ratio, d, n, **query_set) == n
        m.sync()
        m.dev_download(d, got)
        m.dev_free(d)
    return got


@pytest.fixture(scope="module")
def boundary():
    frames = R.planted_frames(900, R.BOUNDARY_SPEC)
    return frames, R.Ref(frames)


class ExternalSet:
    """query frames as a device-resident external query set"""

    def __init__(self, m, queries):
        self.m = m
        stride = max(max(len(r) for _, r in queries), 1)
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


# ---- boundaries ----------------------------------------------------------------------------------------------------------

def test_boundaries(db, pkg, boundary):
    """39 / 40 / 41 rows on either side, planted counts 11 / 12 / 13 under (0.7, 40, 12)."""
    frames, ref = boundary
    fill(db, frames)
    ratio, min_rows, min_matches = R.BOUNDARY_RP
    got, n_pairs = db.all_vs_all_loops_ratio(ratio, min_rows, min_matches)
    want = ref.expected(1, ratio, min_rows, min_matches)
    assert n_pairs == len(ref.pairs(1)) == 55 and 0 < len(want) < n_pairs
    assert_cands(pkg, got, want, "boundaries")
    # launch info: the ratio search's figures, the loop-test kernels as the follow-up
    info = db.launch_info()
    assert info.route == pkg.capi.ROUTE_PLAIN and info.pairs == n_pairs
    assert info.kernel_ms > 0 and info.aux_kernel_ms > 0
    assert info.distances == sum(len(frames[c][1]) * len(frames[s][1]) for c, s in ref.pairs(1))
    # the score array left on the device == a separate all_vs_all_ratio download, byte for byte
    left = db.last_bulk_scores()
    sep = ratio_scores(db, pkg, ratio)
    assert len(left) == n_pairs and left.tobytes() == sep.tobytes()
    # each threshold moves the list as the helper says
    for rp in ((0.7, 41, 12), (0.7, 39, 12), (0.7, 40, 13), (0.7, 40, 11), (0.7, 0, 0), (0.5, 40, 12)):
        got, _ = db.all_vs_all_loops_ratio(*rp)
        assert_cands(pkg, got, ref.expected(1, *rp), f"rp {rp}")


def test_defaults(db, pkg):
    """The reference's own values through rp == NULL: 0.7, 100 rows, 300 matches."""
    frames = R.default_frames()
    ref = R.Ref(frames)
    fill(db, frames)
    got, n_pairs = db.all_vs_all_loops_ratio()                  # all three None: rp = NULL
    want = ref.expected(1, *R.DEFAULTS)
    assert n_pairs == 28 and [(c, m, g) for c, m, g, _ in want] == [(1, 0, 300), (4, 0, 300), (4, 1, 300)]
    assert_cands(pkg, got, want, "defaults")
    explicit, _ = db.all_vs_all_loops_ratio(0.7, 100, 300)
    assert explicit.tobytes() == got.tobytes()
    assert_cands(pkg, db.detect_loops_ratio(4), [w for w in want if w[0] == 4], "defaults, one frame")
    # the 99-row frame passes once min_rows lets it
    got, _ = db.all_vs_all_loops_ratio(0.7, 99, 300)
    assert_cands(pkg, got, ref.expected(1, 0.7, 99, 300), "min_rows 99")
    assert (7, 6) in list(zip(got["current_frame_id"].tolist(), got["matched_frame_id"].tolist()))


# ---- compaction across wave and block boundaries -------------------------------------------------------------------------

@pytest.mark.parametrize("n_pairs", sorted(R.TINY_SHAPES))
def test_compaction(db, pkg, n_pairs):
    """n_pairs = 255, 256, 257, 1025 tiny pairs: every pair a candidate (ranks at every lane of every wave and block, the
    partial last block), then subsets selected by the count and by the rows."""
    nq, ns = R.TINY_SHAPES[n_pairs]
    stored, queries = R.tiny_set(910 + n_pairs, nq, ns)
    ref = R.Ref(stored, queries)
    fill(db, stored)
    ext = ExternalSet(db, queries)
    try:
        for rp in R.TINY_RPS:
            got, n = db.all_vs_all_loops_ratio(*rp, **ext.kw)
            assert n == n_pairs
            want = ref.expected(1, *rp)
            assert_cands(pkg, got, want, f"n_pairs {n_pairs} rp {rp}")
            if rp == (1.0, 0, 0):
                assert len(got) == n_pairs
            assert db.launch_info().aux_kernel_ms > 0
    finally:
        ext.free()


# ---- capacity ------------------------------------------------------------------------------------------------------------

def test_capacity(db, pkg, boundary):
    frames, ref = boundary
    fill(db, frames)
    rp = pkg.capi.RatioLoopParams(*R.BOUNDARY_RP)
    want = ref.expected(1, *R.BOUNDARY_RP)
    count = len(want)
    lib, h = db._lib, db._h
    buf = np.zeros(count + 4, pkg.capi.CANDIDATE_DTYPE)
    raw = buf.view(np.uint8)
    raw[:] = 0xAB
    n, npairs = C.c_size_t(0), C.c_size_t(0)

    def call(out, cap):
        return lib.lcm_all_vs_all_loops_ratio(h, None, None, None, 0, 0, C.byref(rp), out, cap, C.byref(n), C.byref(npairs))

    assert call(buf.ctypes.data_as(C.c_void_p), count - 1) == pkg.capi.ERR_CAPACITY
    assert n.value == count and npairs.value == 55 and (raw == 0xAB).all()
    assert call(None, 100) == pkg.capi.ERR_CAPACITY and n.value == count          # out == NULL with candidates present
    assert call(buf.ctypes.data_as(C.c_void_p), count) == 0 and n.value == count
    assert_cands(pkg, buf[:count], want, "cap == count")
    assert (raw[count * 24:] == 0xAB).all()
    # zero candidates with cap = 0
    rp.min_matches = 14
    assert ref.expected(1, 0.7, 40, 14) == []
    assert call(buf.ctypes.data_as(C.c_void_p), 0) == 0 and n.value == 0
    assert call(None, 0) == 0 and n.value == 0
    # the one-frame form: same refusal, same count
    k = C.c_int32(0)
    rp.min_matches = 12
    mine = [w for w in want if w[0] == 10]
    assert len(mine) >= 2
    raw[:] = 0xAB
    assert lib.lcm_detect_loops_ratio(h, 10, None, 0, C.byref(rp), buf.ctypes.data_as(C.c_void_p), len(mine) - 1, C.byref(k)) == pkg.capi.ERR_CAPACITY
    assert k.value == len(mine) and (raw == 0xAB).all()
    assert lib.lcm_detect_loops_ratio(h, 10, None, 0, C.byref(rp), buf.ctypes.data_as(C.c_void_p), len(mine), C.byref(k)) == 0
    assert_cands(pkg, buf[: k.value], mine, "detect, cap == count")


# ---- min_gap on sparse ids, external query set ---------------------------------------------------------------------------

def test_min_gap_and_external_query_set(db, pkg, boundary):
    _, dense = boundary
    ids = [0, 3, 4, 10, 11, 30, 31, 32, 40, 41, 100]
    frames = [(i, rows) for i, (_, rows) in zip(ids, dense.frames)]
    ref = R.Ref(frames)
    ref.knn = dense.knn                              # same rows, same pair indices
    fill(db, frames)
    db.set_params(min_gap=5)
    rp = R.BOUNDARY_RP
    got, n_pairs = db.all_vs_all_loops_ratio(*rp)
    want = ref.expected(5, *rp)
    assert n_pairs == len(ref.pairs(5)) < 55 and len(want) > 0
    assert_cands(pkg, got, want, "min_gap 5")
    ext = ExternalSet(db, frames)
    try:
        got, n = db.all_vs_all_loops_ratio(*rp, **ext.kw)
        assert n == n_pairs
        assert_cands(pkg, got, want, "external query set")
        # ... and with ids of its own: every stored frame is eligible for every query frame
        far = [(200 + k, rows) for k, (_, rows) in enumerate(frames)]
        ext.kw["q_ids"] = [i for i, _ in far]
        fref = R.Ref(frames, far)
        got, n = db.all_vs_all_loops_ratio(0.7, 40, 12, **ext.kw)
        assert n == 121
        assert_cands(pkg, got, fref.expected(5, 0.7, 40, 12), "external, own ids")
    finally:
        ext.free()


# ---- parameters that play no part, alternation ---------------------------------------------------------------------------

def test_other_parameters_are_ignored(db, pkg, boundary):
    frames, ref = boundary
    fill(db, frames)
    want = ref.expected(1, *R.BOUNDARY_RP)
    db.set_params(ratio=7, dist_floor=99, min_matches=1, sim_threshold=0.9)
    db.set_kernel_variant(1)
    got, _ = db.all_vs_all_loops_ratio(*R.BOUNDARY_RP)
    assert_cands(pkg, got, want, "params")
    assert_cands(pkg, db.detect_loops_ratio(10, None, *R.BOUNDARY_RP), [w for w in want if w[0] == 10], "params, one frame")


def test_alternates_with_the_other_bulk_calls(db, pkg, boundary):
    frames, ref = boundary
    fill(db, frames)
    db.set_params(min_matches=5, sim_threshold=0.05)
    first, n1 = db.all_vs_all_loops(cap=64)
    first, scores1 = first.copy(), db.last_bulk_scores()
    before = ratio_scores(db, pkg, 0.7)
    got, _ = db.all_vs_all_loops_ratio(*R.BOUNDARY_RP)
    after = ratio_scores(db, pkg, 0.7)
    third, n3 = db.all_vs_all_loops(cap=64)
    assert n1 == n3 == 55 and first.tobytes() == third.tobytes() and len(first) > 0
    assert scores1.tobytes() == db.last_bulk_scores().tobytes()
    assert before.tobytes() == after.tobytes()
    assert_cands(pkg, got, ref.expected(1, *R.BOUNDARY_RP), "between two all_vs_all_loops")
    again, _ = db.all_vs_all_loops_ratio(*R.BOUNDARY_RP)
    assert again.tobytes() == got.tobytes()


# ---- the one-frame form --------------------------------------------------------------------------------------------------

def test_detect_loops_ratio(db, pkg, boundary):
    frames, ref = boundary
    fill(db, frames)
    rp = R.BOUNDARY_RP
    bulk, _ = db.all_vs_all_loops_ratio(*rp)
    for cur in (2, 5, 10):
        rows = frames[cur][1]
        mine = bulk[bulk["current_frame_id"] == cur]
        host = db.detect_loops_ratio(cur, rows, *rp)
        stored = db.detect_loops_ratio(cur, None, *rp)
        assert host.tobytes() == stored.tobytes() == mine.tobytes(), cur
        assert_cands(pkg, host, ref.expected(1, *rp, only_query=cur), f"frame {cur}")
    assert len(bulk[bulk["current_frame_id"] == 10]) > 0 and len(bulk[bulk["current_frame_id"] == 5]) == 0
    # a ticket outstanding from query_submit stays collectable and unchanged
    q = frames[10][1]
    plain_scores, plain_ids = db.query_scores(q, 10)
    t = db.query_submit(q, 10)
    beside = db.detect_loops_ratio(10, None, *rp)
    s2, i2 = db.query_collect(t)
    np.testing.assert_array_equal(s2, plain_scores)
    np.testing.assert_array_equal(i2, plain_ids)
    assert beside.tobytes() == bulk[bulk["current_frame_id"] == 10].tobytes()
    # an id that is not stored: with rows it is just a frame id, without it is an error
    with pytest.raises(pkg.LcmError) as e:
        db.detect_loops_ratio(77, None, *rp)
    assert e.value.code == pkg.capi.ERR_NOT_FOUND
    far = db.detect_loops_ratio(77, q, *rp)
    assert_cands(pkg, far, [(77, m, g, s) for _, m, g, s in R.Ref(frames, [(77, q)]).expected(1, *rp)], "host rows, new id")
    # nothing eligible; an explicit empty frame
    assert len(db.detect_loops_ratio(0, None, *rp)) == 0
    assert len(db.detect_loops_ratio(0, q, *rp)) == 0
    assert len(db.detect_loops_ratio(50, np.zeros((0, 32), np.uint8), *rp)) == 0


# ---- errors ----------------------------------------------------------------------------------------------------------------

def test_errors(db, pkg):
    m, E = db, pkg.capi
    rng = np.random.default_rng(950)
    q, t = R.rnd(rng, 20), R.rnd(rng, 30)
    fill(m, [(0, t), (1, q)])

    def code(fn, *a, **kw):
        with pytest.raises(pkg.LcmError) as e:
            fn(*a, **kw)
        return e.value.code

    for bad in (dict(ratio=float("nan")), dict(ratio=-1.0), dict(min_rows=-1), dict(min_matches=-1)):
        assert code(m.all_vs_all_loops_ratio, **bad) == E.ERR_INVALID_ARG, bad
        assert code(m.detect_loops_ratio, 1, None, **bad) == E.ERR_INVALID_ARG, bad
        assert code(m.detect_loops_ratio, 1, q, **bad) == E.ERR_INVALID_ARG, bad
    m.set_params(cross_check=1)
    try:
        assert code(m.all_vs_all_loops_ratio) == E.ERR_INVALID_ARG
        assert code(m.detect_loops_ratio, 1) == E.ERR_INVALID_ARG
    finally:
        m.set_params(cross_check=0)
    assert m.all_vs_all_loops_ratio(0.7, 0, 0)[1] == 1
    # a query frame above 2048 rows
    big = R.rnd(rng, 2049)
    assert code(m.detect_loops_ratio, 2, big) == E.ERR_CAPACITY
    m.append(2, big)
    assert code(m.all_vs_all_loops_ratio) == E.ERR_CAPACITY
    assert code(m.detect_loops_ratio, 2) == E.ERR_CAPACITY
    m.truncate(2)
    m.append(2, big[:2048])
    assert m.all_vs_all_loops_ratio(0.7, 0, 0)[1] == 3

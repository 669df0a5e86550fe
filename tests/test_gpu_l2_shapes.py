"""The SIFT / L2 pair mode's two kernel shapes, its rescan path and its limits (lcm_l2.hip / lcm_l2.cpp) against
tests/l2ref.py — indices, float32 distance BITS and squared distances, all exact.  Needs a real MI355X.

test_gpu_l2.py reaches k_l2_score<2> (256-row chunks, two query tiles per wave) through one ratio-filtered pairs call and
k_l2_rescan through job 0 at the first collision only.  Here LCM_TUNE_L2_CHUNK (read on every call) pins each shape in
turn and every call asserts the shape that served it; the inputs are tests/l2cases.py's (collision table, high-distance
sets, tall cases) and test_gpu_l2.py's own edge cases."""
import numpy as np
import pytest

import knnref
import l2cases as L
import l2ref
import test_gpu_l2 as base

pytestmark = pytest.mark.gpu

TILE, SEG, AUTO_LARGE_ITEMS = 32, 512, 1024
NQ = base.NQ + (255, 256, 511, 512, 513, 600)                     # two and three 256-row chunks; waves with 2, 1 or no tile
NT = base.NT
BIG = 1e30                                                          # a ratio that keeps every row with two neighbours


def items(nq, nt, ch):
    return -(-nq // ch) * -(-nt // SEG)


@pytest.fixture(params=(128, 256))
def chunk(request, monkeypatch):
    monkeypatch.setenv("LCM_TUNE_L2_CHUNK", str(request.param))
    return request.param


@pytest.fixture
def auto(monkeypatch):
    monkeypatch.delenv("LCM_TUNE_L2_CHUNK", raising=False)


def auto_chunk(pairs):
    return 128 if sum(items(nq, nt, 256) for nq, nt in pairs) < AUTO_LARGE_ITEMS else 256


def check(matcher, ch, q, t, msg="", ref=None, dsq=None):
    """knn2_pair_l2 == reference, bit for bit, and the call ran with chunks of `ch` rows."""
    got = matcher.knn2_pair_l2(q, t)
    assert matcher.launch_info().workgroups == items(len(q), len(t), ch), (msg, ch)
    base.assert_knn(got, l2ref.knn2(q, t, dsq) if ref is None else ref, f"{msg} chunk {ch}")
    assert got[0].size == 0 or got[0].max() < len(t), msg
    return got


def expect_list(ref, ratio):
    return base.as_list(*l2ref.ratio_filter(ref[0], ref[1], ratio))


# ---- both shapes, neighbour by neighbour ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shapes():
    rng = np.random.default_rng(2025)
    q, t = base.rnd(rng, max(NQ)), base.rnd(rng, max(NT))
    t[[0, 31, 32, 511, 512, 1024]] = q[[0, 255, 256, 257, 512, 599]]   # exact matches from both tiles of a wave, every chunk
    D = l2ref.distances_sq(q, t)
    L.ro(q, t, D)
    return q, t, D


@pytest.mark.parametrize("nt", NT)
def test_shapes(matcher, shapes, chunk, nt):
    q, t, D = shapes
    for nq in NQ:
        idx, dist, dsq = check(matcher, chunk, q[:nq], t[:nt], f"{nq} x {nt}", dsq=np.ascontiguousarray(D[:nq, :nt]))
        assert idx.shape == (nq, 2)
        if nt == 1:
            assert (idx[:, 1] == -1).all() and np.isposinf(dist[:, 1]).all() and (dsq[:, 1] == 0xFFFFFFFF).all()


def test_query_rows_do_not_leak_between_the_tiles_of_a_wave(matcher, chunk):
    """Rows 0..31 and 32..63 share a wave under 256-row chunks: their norms differ by orders of magnitude here, so the
    second tile scored with the first tile's |q|^2 (or the other way round) is wrong everywhere."""
    rng = np.random.default_rng(21)
    q = np.concatenate([base.rnd(rng, 32, 8), base.rnd(rng, 32) | np.uint8(0xC0), base.rnd(rng, 32, 8), base.rnd(rng, 37) | np.uint8(0xC0)] * 3)
    t = base.rnd(rng, SEG + 70)
    check(matcher, chunk, q, t, "mixed norms")
    check(matcher, chunk, q[:97], t[:TILE + 5], "mixed norms, partial tile")


@pytest.mark.parametrize("nt", (1, 2, 3, 4, 5, 9, TILE + 1, SEG + 1))
def test_identical_train_rows(matcher, chunk, nt):
    rng = np.random.default_rng(100 + nt)
    idx, _, _ = check(matcher, chunk, base.rnd(rng, 300), np.repeat(base.rnd(rng, 1), nt, axis=0))
    assert (idx[:, 0] == 0).all() and (idx[:, 1] == (1 if nt > 1 else -1)).all()


@pytest.mark.parametrize("where", ((TILE - 1, TILE), (SEG - 1, SEG), (0, 2 * SEG), (SEG, SEG + TILE), (TILE, SEG - 1, SEG, SEG + 1)))
def test_duplicates_of_the_best_row_across_boundaries(matcher, chunk, where):
    rng = np.random.default_rng(sum(where))
    q, t = base.rnd(rng, 300), base.rnd(rng, 2 * SEG + 5)
    rows = (3, 40, 130, 170, 299)                                   # first and second tile of a wave, both chunks
    q[list(rows)] = q[3]
    t[list(where)] = q[3]
    idx, _, dsq = check(matcher, chunk, q, t)
    for r in rows:
        assert idx[r].tolist() == list(where[:2]) and dsq[r].tolist() == [0, 0]


@pytest.mark.parametrize("nt", (5, 6, 7, TILE + 1, TILE + 2, TILE + 3, SEG + 1, SEG + 2, SEG + 3, SEG + TILE + 1))
def test_last_row_is_the_best(matcher, chunk, nt):
    """test_gpu_l2.py's padding trap with query rows in BOTH tiles of every wave (the checked epilogue runs for j = 0 and
    j = 1) and in a second chunk."""
    rng = np.random.default_rng(nt)
    x = base.rnd(rng, 1)
    q = np.repeat(x, 290, axis=0)
    t = np.repeat(255 - x, nt, axis=0)
    t[np.arange(nt - 1), rng.integers(0, 128, nt - 1)] ^= np.uint8(1)
    t[nt - 1] = x
    idx, _, _ = check(matcher, chunk, q, t)
    assert (idx[:, 0] == nt - 1).all() and (idx[:, 1] < nt - 1).all()
    check(matcher, chunk, np.zeros((70, 128), np.uint8), t)
    check(matcher, chunk, np.full((70, 128), 128, np.uint8), t)


def test_byte_extremes(matcher, chunk):
    rng = np.random.default_rng(11)
    ext = base.extreme_rows(rng)
    pool = np.concatenate([ext, base.rnd(rng, 30)] * 5)              # 220 rows: the extremes in both tiles of a wave
    check(matcher, chunk, ext, ext, "extremes x extremes")
    check(matcher, chunk, pool, ext[::-1].copy(), "pool x extremes")
    check(matcher, chunk, ext, pool[rng.permutation(len(pool))], "extremes x pool")
    check(matcher, chunk, pool, pool[rng.permutation(len(pool))], "pool x pool")
    _, _, dsq = check(matcher, chunk, ext[:1], ext[1:2].repeat(3, axis=0), "0 x 255")
    assert (dsq == l2ref.MAX_D).all()


# ---- the rescan: sqrtf's classes, non-zero queries, more rows than waves ---------------------------------------------------

def test_collision_table(matcher, chunk):
    for c in L.collision_cases():
        idx, dist, dsq = check(matcher, chunk, c.query, c.train, f"c {c.c} D {c.D} rows {c.lo} {c.hi}")
        assert (idx == c.want).all()


def test_collision_table_at_the_last_rows_of_a_65535_row_matrix(matcher, chunk):
    n = 0
    for c, ref in L.tall_collision_cases():
        idx, _, _ = check(matcher, chunk, c.query, c.train, f"c {c.c} D {c.D}", ref=ref)
        assert (idx == c.want).all() and max(c.want) >= 65533
        n += 1
    assert n >= 4


@pytest.fixture(scope="module")
def high_sets():
    sets = {"offsets": L.high_offsets(), "random": L.high_random(1100, 200, seed=3), "binary": L.high_binary(),
            "random wide": L.high_random(70, SEG + 60, seed=8)}
    return {k: (s, l2ref.knn2(s.query, s.train)) for k, s in sets.items()}


@pytest.mark.parametrize("name", ("offsets", "random", "binary", "random wide"))
def test_high_distance_sets(matcher, chunk, high_sets, name):
    s, ref = high_sets[name]
    check(matcher, chunk, s.query, s.train, name, ref=ref)
    if name == "offsets":
        assert len(s.query) * s.flagged_share > 1024 + 400 and s.n_reordered >= 150    # more flagged rows than waves


# ---- tall cases ---------------------------------------------------------------------------------------------------------------

TALL = {"train 0": lambda: L.tall_train(0), "train 1": lambda: L.tall_train(1), "trap": L.tall_trap,
        "query 33": lambda: L.tall_query(33), "query 513": lambda: L.tall_query(513)}


@pytest.fixture(scope="module")
def tall_cases():
    """Each case and its reference are made once, when the first test asks for them."""
    made = {}
    return lambda name: made[name] if name in made else made.setdefault(name, TALL[name]())


@pytest.mark.parametrize("name", ("train 0", "train 1", "trap", "query 33", "query 513"))
@pytest.mark.parametrize("pin", (None, 256))
def test_tall(matcher, monkeypatch, tall_cases, name, pin):
    c = tall_cases(name)
    if pin is None:
        monkeypatch.delenv("LCM_TUNE_L2_CHUNK", raising=False)
        ch = auto_chunk([(len(c.query), len(c.train))])
        assert ch == 128                                            # every tall call stays below 1024 items of 256 rows
    else:
        monkeypatch.setenv("LCM_TUNE_L2_CHUNK", str(pin))
        ch = pin
    idx, _, dsq = check(matcher, ch, c.query, c.train, name, ref=c.ref)
    if name.startswith("train"):
        for r, want_idx, want_d in c.plants:
            assert idx[r].tolist() == want_idx and dsq[r].tolist() == want_d
        ratio_list = matcher.match_features_ratio_l2(c.query, c.train, 0.75)
        base.assert_same_list(ratio_list, expect_list(c.ref, 0.75), name)


# ---- the rescan inside the pairs call: later jobs, both shapes -------------------------------------------------------------

@pytest.fixture(scope="module")
def rescan_pairs():
    """Frames: one constant query frame per c, two random frames that need no rescan, then the collision cases' train
    matrices.  Pairs: the random ones first, then every collision case, then both again in another order."""
    rng = np.random.default_rng(31)
    cases = L.collision_cases()
    nq = 70                                                         # three tiles: both tiles of wave 0 and one of wave 1
    frames = [np.full((nq, 128), c, np.uint8) for c in L.CONSTANTS] + [base.rnd(rng, 90), base.rnd(rng, 300)]
    qf = {c: k for k, c in enumerate(L.CONSTANTS)}
    plain = [(3, 4), (4, 3), (3, 3)]
    pairs = list(plain)
    for c in cases:
        frames.append(c.train)
        pairs.append((qf[c.c], len(frames) - 1))
    pairs += plain[::-1] + pairs[len(plain):][::-1]
    refs = {p: l2ref.knn2(frames[p[0]], frames[p[1]]) for p in set(pairs)}
    for p in plain:
        assert (refs[p][2][:, 1] < L.RESCAN).all()                  # no rescan for these
    for c, p in zip(cases, pairs[len(plain):]):
        assert (refs[p][0] == c.want).all() and (refs[p][2][:, 1] >= L.RESCAN).all()
    return frames, pairs, refs


@pytest.mark.parametrize("repeat", (1, 5))
def test_rescan_in_the_pairs_call(matcher, chunk, rescan_pairs, repeat):
    frames, pairs, refs = rescan_pairs
    pairs = pairs * repeat
    for ratio in (BIG, 0.75, 1.0):
        lists, offs = matcher.match_pairs_ratio_l2(frames, pairs, ratio)
        assert matcher.launch_info().workgroups == sum(items(len(frames[a]), len(frames[b]), chunk) for a, b in pairs)
        for k, p in enumerate(pairs):
            base.assert_same_list(lists[k], expect_list(refs[p], ratio), f"pair {k} {p} ratio {ratio}")
        if ratio == BIG:
            assert all(len(lists[k]) == len(frames[p[0]]) for k, p in enumerate(pairs))


def test_rescan_in_the_pairs_call_automatic_shapes(matcher, auto, rescan_pairs):
    """The automatic choice: 128-row chunks below 1024 items, 256-row chunks from there on."""
    frames, pairs, refs = rescan_pairs
    n1 = sum(items(len(frames[a]), len(frames[b]), 256) for a, b in pairs)
    assert n1 < AUTO_LARGE_ITEMS <= 4 * n1
    for rep, ch in ((1, 128), (4, 256)):
        many = pairs * rep
        lists, _ = matcher.match_pairs_ratio_l2(frames, many, BIG)
        assert matcher.launch_info().workgroups == sum(items(len(frames[a]), len(frames[b]), ch) for a, b in many)
        for k, p in enumerate(many):
            base.assert_same_list(lists[k], expect_list(refs[p], BIG), f"pair {k} {p}")


# ---- more pairs in one call than gridDim.y holds ----------------------------------------------------------------------------

N_MANY = 70_000


def test_70000_pairs_in_one_l2_call(matcher, auto):
    """Jobs past 65535: the fold goes out in slices, and the rescan finds a later slice's job by its index in the call."""
    z = np.zeros((1, 128), np.uint8)
    coll = np.stack([l2ref.row_with_dsq(base.COLL + 1), l2ref.row_with_dsq(base.COLL)])      # wants [0, 1] after the rescan
    rng = np.random.default_rng(41)
    frames = [z, coll, base.rnd(rng, 3), np.concatenate([base.rnd(rng, 1), 255 - z])]
    assert [len(f) for f in frames] == [1, 2, 3, 2]
    combos = [(a, b) for a in range(4) for b in range(4)]
    pairs = np.array([combos[(k * 7) % 16] for k in range(N_MANY)], np.int32)
    refs = {p: l2ref.knn2(frames[p[0]], frames[p[1]]) for p in combos}
    assert refs[(0, 1)][0].tolist() == [[0, 1]] and refs[(0, 1)][2].tolist() == [[base.COLL + 1, base.COLL]]
    want = {p: expect_list(refs[p], BIG) for p in combos}
    lists, offs = matcher.match_pairs_ratio_l2(frames, pairs, BIG)
    info = matcher.launch_info()
    assert info.pairs == N_MANY and info.workgroups == N_MANY
    counts = np.array([len(want[tuple(p)]) for p in pairs.tolist()])
    np.testing.assert_array_equal(np.asarray(offs, np.int64), np.concatenate([[0], np.cumsum(counts)]))
    got = np.concatenate(lists)
    base.assert_same_list(got, np.concatenate([want[tuple(p)] for p in pairs.tolist()]), "all lists")
    for k in (0, 1, 65534, 65535, 65536, 65537, N_MANY - 1):
        base.assert_same_list(lists[k], want[tuple(pairs[k])], f"pair {k}")
    last = np.nonzero((pairs == (0, 1)).all(1))[0][-1]
    assert last > 65536 and lists[last]["train_idx"].tolist() == [0]   # the collision order in a job of the second slice


def test_70000_pairs_in_one_stored_batch_call(matcher):
    m = matcher
    m.clear()
    try:
        rng = np.random.default_rng(42)
        stored = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in (1, 2, 3, 5)]
        stored[3][4] = stored[2][1]
        for fid, rows in enumerate(stored):
            m.append(fid, rows)
        combos = [(a, b) for a in range(4) for b in range(4)]
        pairs = np.array([combos[(k * 5) % 16] for k in range(N_MANY)], np.int32)
        want = {}
        for p in combos:
            idx, dist = knnref.knn2(stored[p[0]], stored[p[1]])
            want[p] = base.as_list(*knnref.ratio_filter(idx, dist, BIG))
        lists, offs = m.match_stored_batch_ratio(pairs, BIG, cap=5 * N_MANY)
        assert m.launch_info().pairs == N_MANY
        counts = np.array([len(want[tuple(p)]) for p in pairs.tolist()])
        np.testing.assert_array_equal(np.asarray(offs, np.int64), np.concatenate([[0], np.cumsum(counts)]))
        got, exp = np.concatenate(lists), np.concatenate([want[tuple(p)] for p in pairs.tolist()])
        for f in base.FIELDS:
            np.testing.assert_array_equal(got[f], exp[f], err_msg=f)
        # the k = 1 fold takes the same slices
        lists1, _ = m.match_stored_batch(pairs, cap=5 * N_MANY)
        for k in (0, 65535, 65536, N_MANY - 1):
            a, b = (int(x) for x in pairs[k])
            ref_list, _ = m.match_features(stored[a], stored[b])
            assert lists1[k].tobytes() == ref_list.tobytes(), k
    finally:
        m.clear()

"""The size-limit generators (tests/limitcases.py) hold what they promise — checked without a GPU: the planted rows are
first minima at the planted distances, a generator that loses an edge fails, the oracle's records show the planted
pairs (min_d, good rows, the pair beyond 15 / 31 bits, the pair with min_d > 128), the tuned oracle equals the scalar
one on blocks cropped around planted rows, and the numpy scan of the wide case equals oracle.bf_match on a crop."""
import numpy as np
import pytest

import limitcases as L


@pytest.fixture(scope="module")
def tall():
    return L.tall_set()                     # runs check_tall


def test_tall_set_layout(tall):
    assert sorted(tall.counts.tolist()) == sorted(L.TALL_ROWS) and tall.stride_rows == L.MAX_ROWS
    assert {65535, 65534, 65533, 65532, 65531, 32768, 32769, 2049, 2000, 0} <= set(tall.counts.tolist())
    assert sum(p.decoy is not None for p in tall.plants) >= 20
    # rows above a frame's count are zero: nothing of a longer neighbour leaks into a cropped read
    for f in range(tall.n_frames):
        assert not tall.rows[f, int(tall.counts[f]):].any()


@pytest.mark.parametrize("side,edge", [("q", 32768), ("t", 2048), ("q", 65534), ("t", 65531)])
def test_tall_set_without_an_edge_fails(side, edge):
    q = tuple(e for e in L.Q_EDGES if not (side == "q" and e == edge))
    t = tuple(e for e in L.T_EDGES if not (side == "t" and e == edge))
    with pytest.raises(AssertionError):
        L.tall_set(q_edges=q, t_edges=t)


def test_tall_set_with_a_moved_decoy_fails(tall):
    """The first-minimum assertion is live: a duplicate BEFORE a planted train row takes the tie, and check_tall says so."""
    p = next(p for p in tall.plants if p.decoy is not None and p.tr >= 10)
    saved = tall.rows[p.tf, p.tr - 5].copy()
    try:
        tall.rows[p.tf, p.tr - 5] = tall.rows[p.tf, p.tr]
        with pytest.raises(AssertionError):
            L.check_tall(tall)
    finally:
        tall.rows[p.tf, p.tr - 5] = saved
    L.check_tall(tall)


def test_expected_records_show_the_planted_pairs(tall, oracle):
    pq, pt, offs = L.tall_pairs(tall)
    sc, sums = oracle.fast_score_pairs_idx(tall.rows, tall.counts, pq, pt, oracle.default_params(min_gap=1), n_threads=16)
    L.check_expected(tall, pq, pt, sc, sums)
    # an empty frame on either side: the empty record
    for k, (q, t) in enumerate(zip(pq, pt)):
        if tall.counts[q] == 0 or tall.counts[t] == 0:
            assert (int(sc[k]["good_count"]), int(sc[k]["min_dist"]), int(sums[k])) == (0, 0xFFFF, 0)


def test_tuned_oracle_equals_scalar_on_crops_around_planted_rows(tall, oracle):
    blocks = L.crop_blocks(tall)
    assert len(blocks) >= 4
    p = oracle.default_params(min_gap=1)
    for plant, q, t, q0, t0 in blocks:
        rows = np.zeros((2, len(t), 32), np.uint8)
        rows[0, : len(q)] = q
        rows[1] = t
        sc, sums = oracle.fast_score_pairs_idx(rows, np.array([len(q), len(t)], np.int32), [0], [1], p, n_threads=1)
        assert sc[0] == oracle.pair_score(q, t, p)
        assert int(sums[0]) == oracle.index_sum(q, t, p)
        idx, dist = oracle.bf_match(q, t)               # the planted row inside the crop
        assert (int(idx[plant.qr - q0]), int(dist[plant.qr - q0])) == (plant.tr - t0, plant.k)


def test_wide_scan_equals_bf_match_on_a_crop(oracle):
    winners = ((0, 7, 0), (4095, 5, 0), (2047, 9, 0), (2048, 9, 0), (1500, 0, 0), (3000, 9, -1000), (3500, 9, +500))
    case = L.wide_case(seed=77, winners=winners, n_extra=24, nt=4096)
    idx, dist = L.wide_scan(case)
    oi, od = oracle.bf_match(case.query, case.train)
    np.testing.assert_array_equal(idx, oi)
    np.testing.assert_array_equal(dist, od)
    np.testing.assert_array_equal(idx, case.want_idx)
    np.testing.assert_array_equal(dist, case.want_dist)
    assert int(idx[5]) == 2000 and int(idx[6]) == 3500          # the earlier duplicate wins, the later one does not


def test_wide_case_holds_its_winners():
    case = L.wide_case()
    assert case.train.shape == (L.WIDE_NT, 32) and L.WIDE_NT == 1 << 22
    named = list(range(len(L.WIDE_WINNERS)))                  # the named winners; the GPU test scans every row
    idx, dist = L.wide_scan(case, named)
    np.testing.assert_array_equal(idx, case.want_idx[named])
    np.testing.assert_array_equal(dist, case.want_dist[named])
    for drop in (4, 8, 9):                                     # 2^22 - 1, the high segment boundary, distance 0
        w = tuple(x for i, x in enumerate(L.WIDE_WINNERS) if i != drop)
        with pytest.raises(AssertionError):
            L.wide_case(winners=w)

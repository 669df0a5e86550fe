"""The checker under the good-match filter's parameter grid: `d <= max(ratio * min_d, dist_floor)`.

The GPU tests compare every route with the oracle's tuned path (`fast_score_pairs_idx`); here that path is pinned to
the scalar oracle (`all_vs_all` / `index_sum`) and to the numpy restatement (`npref.pair_score`) at every
(ratio, dist_floor) of the grid, on ragged random frames and on planted frames whose rows sit exactly at thr - 1, thr,
thr + 1 and in the far range (min_d > 128, distances up to 256).  Hand-derived answers pin the rule itself."""
import numpy as np
import pytest

import planted
from npref import pair_score as np_pair_score


def _pairs(ids, gap=1):
    pq, pt = [], []
    for c in range(len(ids)):
        for t in range(len(ids)):
            if ids[c] - ids[t] >= gap:
                pq.append(c); pt.append(t)
    return pq, pt


def _databases(pkg, ratio, floor):
    fs = pkg.synth.make_frames(8, 90, seed=404, ragged=True, dup_frac=0.5)
    fs.counts[3] = 0                                        # an empty frame in the mix
    fs.rows[6, :30] = fs.rows[2, :30]                       # exact duplicates across frames: min_d == 0, ties
    yield "ragged", fs.rows, fs.counts, fs.ids
    pf = planted.frames([("near", 33, 31), ("far", 5, 9), ("near", 64, 65), ("far", 4, 3, "tied"), ("near", 5, 1)],
                        ratio, floor, seed=7)
    yield "planted", pf.rows, pf.counts, pf.ids


@pytest.mark.parametrize("ratio,floor", planted.GRID)
def test_tuned_path_equals_scalar_and_numpy(oracle, pkg, ratio, floor):
    p = oracle.default_params(ratio=ratio, dist_floor=floor, min_gap=1)
    for name, rows, counts, ids in _databases(pkg, ratio, floor):
        scalar, offs = oracle.all_vs_all(rows, counts, ids, p)
        pq, pt = _pairs(ids)
        assert len(scalar) == len(pq) > 0
        for threads in (1, 3):
            fast, sums = oracle.fast_score_pairs_idx(rows, counts, pq, pt, p, n_threads=threads)
            np.testing.assert_array_equal(fast, scalar, err_msg=f"{name} threads={threads}")
            for k, (c, t) in enumerate(zip(pq, pt)):
                q_rows, t_rows = rows[c, : counts[c]], rows[t, : counts[t]]
                assert int(sums[k]) == oracle.index_sum(q_rows, t_rows, p), (name, c, t)
                if threads == 1:
                    s = fast[k]
                    assert (int(s["good_count"]), int(s["min_dist"]), int(s["n_train"])) == \
                        np_pair_score(q_rows, t_rows, ratio, floor), (name, c, t)


@pytest.mark.parametrize("ratio,floor", planted.GRID)
def test_planted_pairs_reach_the_boundary(oracle, ratio, floor):
    """The generator's own promise, seen through the oracle: a planted pair's good_count is the number of rows at or
    below thr, and where thr + 1 is reachable some row sits there and is NOT counted."""
    for pair in (planted.near_pair(65, 64, ratio, floor, 1), planted.far_pair(33, 31, ratio, floor, 1),
                 planted.far_pair(9, 5, ratio, floor, 2, tied=True)):
        best = planted.dist_matrix(pair.q, pair.t).min(axis=1)
        s = oracle.pair_score(pair.q, pair.t, oracle.default_params(ratio=ratio, dist_floor=floor))
        assert int(s["min_dist"]) == pair.min_d
        assert int(s["good_count"]) == int((best <= pair.thr).sum())
        assert np_pair_score(pair.q, pair.t, ratio, floor)[0] == int(s["good_count"])


def _rows_at(distances):
    """Query rows at exactly these distances from ONE all-zero train row (the first d bits set, spread over dwords)."""
    q = np.zeros((len(distances), 32), np.uint8)
    for i, d in enumerate(distances):
        bits = np.zeros(256, np.uint8)
        bits[[(j * 37) % 256 for j in range(d)]] = 1          # 37 is odd: j -> 37 j mod 256 is a permutation
        q[i] = np.packbits(bits, bitorder="little")
    return q, np.zeros((1, 32), np.uint8)


def _score(oracle, q, t, ratio, floor):
    p = oracle.default_params(ratio=ratio, dist_floor=floor, min_gap=1)
    s = oracle.pair_score(q, t, p)
    rows = np.zeros((2, max(len(q), len(t), 1), 32), np.uint8)
    rows[0, : len(t)] = t
    rows[1, : len(q)] = q
    counts = np.array([len(t), len(q)], np.int32)
    fast, _ = oracle.fast_score_pairs_idx(rows, counts, [1], [0], p, n_threads=1)
    assert fast[0] == s
    assert (int(s["good_count"]), int(s["min_dist"]), int(s["n_train"])) == np_pair_score(q, t, ratio, floor)
    return int(s["good_count"]), int(s["min_dist"])


@pytest.mark.parametrize("m,ratio", [(0, 2), (1, 2), (20, 2), (36, 3), (85, 3), (128, 2), (30, 1)])
def test_ratio_boundary_is_inclusive(oracle, m, ratio):
    thr = ratio * m
    ds = [m] + [d for d in (thr, thr + 1) if d <= 256]
    q, t = _rows_at(ds)
    good, md = _score(oracle, q, t, ratio, 0)
    assert md == m
    assert good == sum(d <= thr for d in ds)          # d == ratio * min_d is good, ratio * min_d + 1 is not
    if thr + 1 <= 256:
        assert good == len(ds) - 1


@pytest.mark.parametrize("m,ratio,floor", [(10, 2, 64), (10, 0, 64), (31, 2, 63), (32, 2, 63), (0, 65536, 5), (200, 1, 255)])
def test_floor_takes_over_above_ratio_times_min(oracle, m, ratio, floor):
    thr = max(ratio * m, floor)
    ds = sorted({m, 2 * m, thr - 1, thr, thr + 1, 256} & set(range(m, 257)))
    q, t = _rows_at(ds)
    good, md = _score(oracle, q, t, ratio, floor)
    assert md == m and good == sum(d <= thr for d in ds)


@pytest.mark.parametrize("floor", [0, 1, 5, 256])
def test_ratio_zero_keeps_only_rows_within_the_floor(oracle, floor):
    ds = [0, 1, 4, 5, 6, 100, 255, 256]
    q, t = _rows_at(ds)
    good, md = _score(oracle, q, t, 0, floor)
    assert md == 0 and good == sum(d <= floor for d in ds)
    q, t = _rows_at(ds[1:])                                   # min_d 1: ratio 0 still gives thr = floor
    good, md = _score(oracle, q, t, 0, floor)
    assert md == 1 and good == sum(d <= floor for d in ds[1:])


def test_ratio_65536_and_the_far_range(oracle):
    q, t = _rows_at([0, 1, 256])
    assert _score(oracle, q, t, 65536, 0) == (1, 0)            # 65536 * 0 = 0: only the exact match
    q, t = _rows_at([1, 200, 256])
    assert _score(oracle, q, t, 65536, 0) == (3, 1)
    q, t = _rows_at([129, 256, 255])                          # min_d > 128: 2 * min_d exceeds every distance
    assert _score(oracle, q, t, 2, 0) == (3, 129)
    assert _score(oracle, q, t, 1, 0) == (1, 129)
    assert _score(oracle, q, t, 1, 255) == (2, 129)
    assert _score(oracle, q, t, 0, 256) == (3, 129)


@pytest.mark.parametrize("ratio,floor", planted.GRID)
def test_empty_train_side_has_no_good_match_whatever_the_floor(oracle, ratio, floor):
    q, _ = _rows_at([0, 3, 256])
    t = np.zeros((0, 32), np.uint8)
    p = oracle.default_params(ratio=ratio, dist_floor=floor, min_gap=1)
    s = oracle.pair_score(q, t, p)
    assert (int(s["good_count"]), int(s["min_dist"]), int(s["n_train"])) == (0, 0xFFFF, 0)
    rows = np.zeros((2, 3, 32), np.uint8)
    rows[1] = q
    counts = np.array([0, 3], np.int32)
    for pq, pt in (([1], [0]), ([0], [1])):                  # empty train side, then empty query side
        fast, sums = oracle.fast_score_pairs_idx(rows, counts, pq, pt, p, n_threads=1)
        assert (int(fast[0]["good_count"]), int(fast[0]["min_dist"])) == (0, 0xFFFF) and int(sums[0]) == 0
    good, keep, m = oracle.filter_good(np.zeros(0, np.int32), ratio, floor)
    assert good == 0 and not keep.any()

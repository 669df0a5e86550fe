"""The k = 2 / ratio size-limit generators (tests/knnlimitcases.py) hold what they promise — checked without a GPU: the
planted rows are the two nearest neighbours at the planted distances, a generator that loses an edge fails, knnref.knn2
equals the insertion loop on crops around planted rows and the generators' own full scan on a 4096-row crop, and the
table sets have type pairs on both sides of the verdict."""
import numpy as np
import pytest

import knnlimitcases as K
import knnref
import ratioref


@pytest.fixture(scope="module")
def tall():
    return K.full_tall_set()                # runs check_tall before and after the tall x tall rows are written


@pytest.fixture(scope="module")
def wide():
    return K.wide2_case()                   # 128 MB of train rows: once per module


def test_tall_set_layout_and_trap(tall):
    assert [len(rows) for _, rows in tall.stored()] == [65535, 65534, 65533, 2048, 513, 96]
    assert [i for i, _ in tall.stored()] == [0, 1, 2, 10, 11, 12] and len(tall.refused) == 2049
    assert tall.min_unrelated >= K.FAR
    for t in K.TALL:                        # every trapped row, not only the first: best = the last row at 0, a far second
        T = tall.frames[t]
        idx, dist = knnref.knn2(tall.frames["Y"][list(K.TRAP_ROWS[t])], T)
        assert (idx[:, 0] == len(T) - 1).all() and (dist[:, 0] == 0).all() and (dist[:, 1] >= K.FAR).all()
        assert len(knnref.ratio_filter(idx, dist, 0.7)[0]) == 64
        # what a kernel that took a padding copy or a next-slot row for a neighbour would report: nothing
        hostile = np.concatenate([T, T[-1:], tall.frames[K.NEXT[t]][:2]])
        idx, dist = knnref.knn2(tall.frames["Y"][list(K.TRAP_ROWS[t])], hostile)
        assert len(knnref.ratio_filter(idx, dist, 1.0)[0]) == 0


@pytest.mark.parametrize("drop", ["runner-up", "next-slot"])
def test_tall_set_without_a_planted_edge_fails(drop):
    with pytest.raises(AssertionError):
        K.tall_set(drop=(drop,))


def test_tall_query_cases_and_a_duplicate_moved_before_its_best(tall):
    for nt in (33, 513):
        case = K.tall_query_case(tall, nt)
        assert len(case.train) == nt and len(case.query) == 65535
        assert {f.kind for f in case.found} == {"a", "b"}
    with pytest.raises(AssertionError):
        K.tall_query_case(tall, 513, drop=("duplicate-first",))
    assert {f.qr for f in tall.tall_found} == set(K.TQ_ROWS)
    assert K.tall_x_tall(tall, check=True, write=False) == tall.tall_found          # B holds the rows: the scan finds them again


def test_knn2_equals_the_insertion_loop_on_crops_around_planted_rows(tall):
    n = 0
    for t in K.TALL:
        T = tall.frames[t]
        for f in tall.plants[t]:
            s = K.SMALL[n % 3]
            pos = K.POS[s][f.qr]
            q0 = max(0, min(pos - 4, K.ROWS[s] - 8))
            t0 = max(0, min(f.i1 - 150, len(T) - 300))
            q, tr = tall.frames[s][q0: q0 + 8], T[t0: t0 + 300]
            ai, ad = knnref.knn2(q, tr)
            bi, bd = knnref.insertion_knn2(q, tr)
            np.testing.assert_array_equal(ai, bi)
            np.testing.assert_array_equal(ad, bd)
            assert (int(ai[pos - q0, 0]), int(ad[pos - q0, 0])) == (f.i1 - t0, f.d1)
            if f.kind in "bc":              # the runner-up lies inside the crop
                assert (int(ai[pos - q0, 1]), int(ad[pos - q0, 1])) == (f.i2 - t0, f.d2)
            n += 1
    assert n >= 18


def test_full_scan_equals_knn2_on_a_4096_row_crop():
    named = (("twin", 0, 4095), ("twin", 2047, 2048), ("pair", 100, 7, 300, 9), ("dup", 1000, 11, 2000),
             ("three", 500, 6, 1500, 3500), ("zero", 1234))
    case = K.wide2_case(seed=78, nt=4096, named=named, n_query=24)
    idx, dist = K.wide2_scan(case)
    K.check_wide2_scan(case, idx, dist)
    ri, rd = knnref.knn2(case.query, case.train)
    np.testing.assert_array_equal(idx, ri)
    np.testing.assert_array_equal(dist, rd.astype(np.int32))
    assert idx[5].tolist() == [1000, 2000] and idx[6].tolist() == [500, 1500]       # the later copies lose, in order


def test_wide_case_holds_its_pairs(wide):
    assert wide.train.shape == (K.WIDE_NT, 32) and wide.query.shape == (40, 32) and K.WIDE_NT == 1 << 22
    rows = range(wide.named)                                  # the named pairs; the GPU test scans every row
    idx, dist = K.wide2_scan(wide, rows)
    K.check_wide2_scan(wide, idx, dist, rows)
    assert int(idx.max()) == K.WIDE_NT - 1 and (idx >= K.HALF).any()
    with pytest.raises(AssertionError):                       # a wide runner-up moved into the best's segment
        K.wide2_case(drop=("same-segment",))
    with pytest.raises(AssertionError):                       # ... and a named pair left out
        K.wide2_case(named=K.WIDE2_NAMED[1:])


def test_table_sets():
    ts = K.table_set()
    g7, m7 = ts.table(0.7)
    assert len([k for k in ts.counts if k[2] == 0.7]) == 64              # the 64 combinations, computed once per ratio
    for a in range(8):
        for b in range(8):
            good, dmin = ratioref.ratio_counts(ts.types[a], ts.types[b], 0.7)
            assert (good, dmin, K.TYPE_ROWS[b]) == ts.expected(a, b, 0.7) == (int(g7[a, b]), int(m7[a, b]), K.TYPE_ROWS[b])
    idx, dist = knnref.knn2(ts.types[2], ts.types[2])
    assert dist.tolist() == [[0, 256], [0, 256]] and g7[2, 2] == 2      # a second neighbour at 256, the field's largest value
    idx, dist = knnref.knn2(ts.types[7], ts.types[4])
    assert (dist[:, 0] == dist[:, 1]).any()                   # equal best and second
    assert K.N_SLICE * (K.N_SLICE - 1) // 2 == 1049076 > 1 << 20
    frames = ts.frames(K.N_ONLINE)
    assert len(frames) == 8200 and all(len(rows) == K.TYPE_ROWS[int(K.type_of(s))] for s, rows in frames[:64])

"""The pre-conditions of tests/test_gpu_l2_emit_limits.py, on the CPU: tests/l2emitcases.py's generators hold what they promise
and FAIL when an edge is taken away (a duplicated row in P, a forced edge of the permutation removed, a keypoint of P moved
to the neighbouring row, a prefix cut to 32766 rows, a tall case that is not sparse at the sparse ratio).  The expected
records of the copy pairs are restated row by row and compared with l2ref on crops of P that hold the neighbour."""
import numpy as np
import pytest

import l2cases as L
import l2emitcases as E
import l2ref
import verifylimitcases as V


def test_the_copy_store_holds_what_it_planted():
    s = E.copy_store()
    p, c = s.frames[E.SLOT_P], s.frames[E.SLOT_C]
    assert p.shape == c.shape == (E.N, 128) and (c == p[s.perm]).all()
    for r, v in E.FORCED:
        assert s.perm[r] == v and (c[r] == p[v]).all()
    big = V.big()[0]
    for n in E.PREFIXES:
        k = E.prefix_slot(n)
        assert len(s.frames[k]) == n and (s.frames[k] == c[:n]).all()
        assert E.bits(E.copy_points(k, E.SLOT_P)).tobytes() == E.bits(big[:n]).tobytes()
    assert E.bits(E.copy_points(E.SLOT_C, E.SLOT_P)).tobytes() == E.bits(big).tobytes()
    assert len(s.frames[E.SLOT_EMPTY]) == 0 and (s.frames[E.SLOT_ONE] == p[65534:]).all()
    assert (s.frames[E.SLOT_SMALL] == p[s.src]).all() and s.src.min() > 65000
    # the ragged call: 256 blocks beside 1, 0, 128, 2, 128, 0, 129 and 256; more than 2^17 records, one pair's above 2^15
    counts = [len(E.copy_train(a, b)) for a, b in E.RAGGED_PAIRS]
    assert counts == [65535, 1, 0, 32767, 257, 32768, 0, 32769, 65535] and sum(counts) > 1 << 17
    assert [len(E.copy_train(a, b)) for a, b in E.VERIFY_PAIRS] == [65535, 257, 2017, 0, 4033]
    # the records of the self pair and of the small frames, by l2ref on a crop that holds the neighbour
    for a, b, crop in ((E.SLOT_SMALL, E.SLOT_P, slice(65000, E.N)), (E.SLOT_ONE, E.SLOT_P, slice(65000, E.N))):
        idx, dist, dsq = l2ref.knn2(s.frames[a], s.frames[b][crop])
        assert (idx[:, 0] + crop.start == E.copy_train(a, b)).all() and (dsq[:, 0] == 0).all() and (dsq[:, 1] > 0).all()
    rows = np.array(E.CHECK_ROWS)
    idx, dist, dsq = L.knn2(c[rows], c)
    assert (idx[:, 0] == rows).all() and (dsq[:, 0] == 0).all() and (dsq[:, 1] > 0).all()          # (C, C): row r finds itself
    assert (E.copy_train(E.SLOT_C, E.SLOT_C)[rows] == rows).all()
    # copy_ref under l2ref's filter: every row at every ratio > 0, none at 0
    ref = E.copy_ref(E.prefix_slot(2017), E.SLOT_P)
    for ratio in (1e-30, 0.7, 1.0, 1e30):
        kept, train, d = l2ref.ratio_filter(ref[0], ref[1], ratio)
        assert len(kept) == 2017 and (train == s.perm[:2017]).all() and not d.any()
    assert len(l2ref.ratio_filter(ref[0], ref[1], 0.0)[0]) == 0


def test_each_copy_generator_fails_without_its_edge():
    with pytest.raises(AssertionError, match="65534 distinct rows"):
        E.make_p(dup=(40000, 7))
    for k in range(len(E.FORCED)):
        with pytest.raises(AssertionError, match=rf"perm\[{E.FORCED[k][0]}\] is"):
            E.make_perm(forced=E.FORCED[:k] + E.FORCED[k + 1:])
    perm = E.copy_store().perm
    for r in (0, 32768, 65534):
        with pytest.raises(AssertionError, match="the point record of query row"):
            E.make_keypoints(perm, move=r)
    with pytest.raises(AssertionError, match="no prefix of 32767 rows"):
        E.check_prefixes((2017, 4033, 32766, 32768, 32769))
    with pytest.raises(AssertionError, match="no prefix of 4033 rows"):
        E.check_prefixes((2017, 4032, 32767, 32768, 32769))
    s = E.copy_store()
    with pytest.raises(AssertionError):                          # a permutation that is off by one on a checked row
        wrong = s.perm.copy()
        wrong[[63, 64]] = wrong[[64, 63]]
        E.cross_check(s.frames[E.SLOT_P], s.frames[E.SLOT_C], wrong)


def test_the_random_store_meets_the_ratio_conditions():
    r = E.random_store()
    assert len(r.pairs) == 8 and sum(1 for a, b in r.pairs if len(r.frames[a]) and len(r.frames[b])) == 6
    for k, p in ((0, r.pairs[0]), (1, r.pairs[2])):
        ref = r.refs[p]
        kept = [len(E.survivors(ref, x)) for x in E.RATIOS]
        print(f"pair {p}: survivors at {E.RATIOS}: {kept}; empty blocks at 0.9: {E.empty_blocks(E.survivors(ref, 0.9), E.N)}, "
              f"at {E.SPARSE_RATIO}: {E.empty_blocks(E.survivors(ref, E.SPARSE_RATIO), E.N)}")
        assert kept[0] == E.N and kept[-1] == 0 and kept[0] > kept[1] > kept[2] > kept[3] > 0
    # a case that is dense at the sparse ratio, or that keeps nothing there, is refused
    dense = r.refs[r.pairs[0]]
    idx, dist, dsq = (a.copy() for a in dense)
    dist[::200, 0] = 0                                           # a sure survivor in every block
    with pytest.raises(AssertionError, match="blocks empty"):
        E.check_tall_ratios((idx, dist, dsq), E.N)
    idx, dist, dsq = (a.copy() for a in dense)
    dist[:, 0] = np.maximum(dist[:, 0], (0.95 * dist[:, 1]).astype(np.float32))
    with pytest.raises(AssertionError, match="ratio 0.9 keeps 0 rows"):
        E.check_tall_ratios((idx, dist, dsq), E.N)
    with pytest.raises(AssertionError):                          # a one-row train matrix: no second neighbour anywhere
        E.check_tall_ratios(L.knn2(r.frames[0][:300], r.frames[1][:1]), 300)

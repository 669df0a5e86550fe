"""The ratio-test score's reference (tests/ratioref.py) against first principles, no GPU: the table `d1 < lim[d2]` is the
float64 comparison for every pair of distances, and ratio_counts agrees with batchDistance's insertion loop + the filter."""
import numpy as np
import pytest

import knnref
import ratioref

RATIOS = (0, 0.5, 0.7, 0.75, 0.8, 1.0, 1.5, 1 / 3, float(np.nextafter(0.7, 1)))


@pytest.mark.parametrize("ratio", RATIOS)
def test_table_is_the_double_comparison(ratio):
    lim = ratioref.lim_table(ratio)
    assert lim.shape == (257,) and lim.max() <= 257
    d1 = np.arange(257)
    for d2 in range(257):
        want = d1.astype(np.float64) < np.float64(ratio) * np.float64(d2)
        np.testing.assert_array_equal(d1 < int(lim[d2]), want, err_msg=f"ratio {ratio} d2 {d2}")


def test_table_distinguishes_neighbouring_ratios():
    a, b = ratioref.lim_table(0.7), ratioref.lim_table(float(np.nextafter(0.7, 1)))
    assert (a <= b).all()
    assert ratioref.lim_table(0).max() == 0
    assert ratioref.lim_table(1.0).tolist() == list(range(257))          # d1 < d2


@pytest.mark.parametrize("nq,nt", [(1, 1), (3, 1), (5, 2), (9, 4), (12, 7), (20, 13)])
def test_ratio_counts_agrees_with_the_insertion_loop(nq, nt):
    rng = np.random.default_rng(nq * 101 + nt)
    alphabet = rng.integers(0, 256, (4, 32), dtype=np.uint8)             # few distinct rows: ties everywhere
    alphabet[1] = alphabet[0]; alphabet[1, 0] ^= 1
    q = alphabet[rng.integers(0, 4, nq)]
    t = alphabet[rng.integers(0, 4, nt)]
    ii, dd = knnref.insertion_knn2(q, t)
    for ratio in RATIOS:
        good, dmin = ratioref.ratio_counts(q, t, ratio)
        assert good == len(knnref.ratio_filter(ii, dd, ratio)[0])
        assert dmin == int(dd[:, 0].min())
        if nt == 1:
            assert good == 0


def test_ratio_counts_empty_sides():
    e = np.zeros((0, 32), np.uint8)
    t = np.ones((3, 32), np.uint8)
    assert ratioref.ratio_counts(e, t, 0.7) == (0, 0xFFFF)
    assert ratioref.ratio_counts(t, e, 0.7) == (0, 0xFFFF)
    assert ratioref.ratio_counts(t, t, 1.0) == (0, 0)                    # identical rows: second == best

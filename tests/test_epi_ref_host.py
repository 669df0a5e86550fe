"""tests/epiref.py, the numpy restatement of the essential-matrix RANSAC (include/lcm.h, lcm_epi_*), checked on its own,
and the pre-conditions of tests/test_gpu_epi.py checked with the reference alone: no GPU, no library."""
import numpy as np
import pytest

import epicases as S
import epiref as R


@pytest.mark.parametrize("n", (8, 9, 64, 65, 4000))
def test_sampler_yields_eight_distinct_indices_in_range(n):
    for seed in (0, 0xFFFFFFFF, 7):
        for pair in (0, 70000):
            for it in range(64):
                s = R.sample8(seed, pair, it, n)
                assert len(s) == 8 and len(set(s)) == 8 and min(s) >= 0 and max(s) < n, (n, seed, pair, it, s)
                if n == 8:
                    assert sorted(s) == list(range(8))


def test_hash_is_32_bit_and_depends_on_every_counter():
    base = R.epi_hash(1, 2, 3, 4)
    assert 0 <= base <= R.M32
    assert len({base, R.epi_hash(0, 2, 3, 4), R.epi_hash(1, 0, 3, 4), R.epi_hash(1, 2, 0, 4), R.epi_hash(1, 2, 3, 0)}) == 5
    assert R.epi_hash(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 7) <= R.M32
    assert R.fmix32(0) == 0 and R.fmix32(1) == 0x514E28B7          # MurmurHash3's finaliser


def test_rule_on_exact_integer_cases():
    E, pts = S.integer_cases()
    k = S.K_UNIT
    a, b, c, d = R.normalise(pts, k)
    got = R.inliers(E, a, b, c, d, R.threshold2(1.0, k))
    np.testing.assert_array_equal(got, pts[:, 1] == pts[:, 3])
    assert 0 < got.sum() < len(pts)
    assert R.counts(np.zeros(9), pts, 1.0, k)[0] == 0                 # the all-zero matrix: den == 0


def test_planted_inliers_pass_under_the_true_matrix():
    for name, n_in, n_out, _ in S.VERIFY_SCENES + (S.RATIO_SCENE, S.SOLVER_SCENE):
        pts, planted = S.scene(name)
        if len(pts) == 0:
            continue
        a, b, c, d = R.normalise(pts)
        inl = R.inliers(R.E_TRUE, a, b, c, d, R.threshold2())
        assert inl[planted].all() and planted.sum() == n_in and len(pts) == n_in + n_out, name


def test_solver_on_the_manifold_and_selection_takes_the_first_of_equals():
    pts, planted = S.scene("noise_free")
    s, E = R.hypotheses(pts, 0, 0, 64)
    assert R.singular_deviation(E).max() < 1e-13
    good = planted[s].all(axis=1)
    assert good.any() and R.truth_distance(E[good]).max() < 0.05
    assert R.select(np.array([3, 9, 9, 2])) == 1 and R.select(np.zeros(5, int)) == 0


@pytest.mark.parametrize("seed", S.SEEDS)
def test_preconditions_of_the_gpu_scenes(seed):
    """Every scene of the GPU tests, with the reference alone: the RANSAC finds at least the planted inliers (and its mask
    covers them), a pure-outlier scene stays at or below min_inliers, the two 400-point scenes fall on the intended sides of
    the loop test."""
    for pair, (name, n_in, n_out, _) in enumerate(S.VERIFY_SCENES):
        pts, planted = S.scene(name)
        n, best, E, mask = S.reference_ransac(name, seed, pair)
        if len(pts) < 8:
            assert (n, best) == (0, 0) and not mask.any()
            continue
        assert n >= n_in and mask[planted].all() and mask.sum() == n, (name, n, n_in)
        if name in S.PURE_OUTLIER:
            assert n <= 200 and not R.loop_test(n, len(pts))
        if name == "eight":
            assert (n, best) == (8, 0)                                # every hypothesis counts 8: the first wins
    n, *_ = S.reference_ransac("s400_280", seed, 0)
    assert R.loop_test(n, 400)
    n, _, _, mask = S.reference_ransac(S.RATIO_SCENE[0], seed, 0)
    assert n >= 230 and mask[S.scene(S.RATIO_SCENE[0])[1]].all()
    assert n > 200 and n / 400 <= 0.6 and not R.loop_test(n, 400)      # fails on the ratio alone

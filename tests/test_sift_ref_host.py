"""The numpy restatement of the SIFT keypoint detector (tests/siftref.py) on its own, without a device: plan values worked by hand,
the taps' symmetry and sum, the fold against a brute-force mirror walk, a constant image, an isotropic blob scene, and the
generators of tests/siftcases.py (each asserts what it planted)."""
import math

import numpy as np
import pytest

import siftcases as S
import siftref as R

# An isotropic blob gives one keypoint, at its centre up to the sampling: the largest distance the restatement shows on
# siftcases.BLOBS is 0.36 pixels (0.24 in x and in y, from the half-pixel shift of the enlarged first octave and the rounding to
# uint8); half a pixel a coordinate is the bound, since a refined offset is below 0.5 by definition.
BLOB_MAX_DISTANCE = 0.5 * math.sqrt(2.0)


def test_plan_values_worked_by_hand():
    p = R.params()
    pl = R.plan(640, 480, p)
    # base 1280 x 960: log2(960) - 2 = 7.9 -> 8, + 1 for the enlarged octave
    assert (pl.n_octaves, pl.n_gauss, pl.n_dog, pl.base_w, pl.base_h) == (9, 6, 5, 1280, 960)
    assert pl.width == [1280, 640, 320, 160, 80, 40, 20, 10, 5] and pl.height == [960, 480, 240, 120, 60, 30, 15, 7, 3]
    k = 2.0 ** (1.0 / 3.0)
    assert pl.sig[0] == 1.6 and abs(pl.sig[1] - 1.6 * math.sqrt(k * k - 1.0)) < 1e-12 and abs(pl.sig[5] - 1.6 * k ** 4 * math.sqrt(k * k - 1.0)) < 1e-12
    # radius = (cvRound(8 sig + 1) | 1) / 2: sig[1] = 1.2263 -> cvRound(10.81) = 11 -> 5; sig[5] = 3.0901 -> 26 | 1 = 27 -> 13
    assert pl.radius == [0, 5, 6, 8, 10, 13] and abs(pl.first_sigma - math.sqrt(1.6 * 1.6 - 1.0)) < 1e-15 and pl.first_radius == 5
    q = R.plan(17, 13, R.params(upsample=0))                 # log2(13) - 2 = 1.70 -> 2
    assert (q.n_octaves, q.width, q.height) == (2, [17, 8], [13, 6]) and abs(q.first_sigma - math.sqrt(1.6 * 1.6 - 0.25)) < 1e-15
    assert R.plan(64, 64, p).n_octaves == 6 and R.plan(64, 64, p).width[-1] == 4
    assert R.plan(64, 64, R.params(n_octaves=3)).n_octaves == 3
    assert R.plan(5, 5, R.params(upsample=0)) is None        # log2(5) - 2 = 0.32 -> no octave
    assert R.plan(4097, 64, p) is None and R.plan(4096, 4096, p).n_octaves == 12
    assert R.plan(64, 64, R.params(n_octave_layers=1)).radius == [0, 11, 22, 45]
    assert R.plan(64, 64, R.params(n_octave_layers=1, sigma=2.0)) is None                  # a radius of 56
    assert R.plan(8, 8, R.params(n_octaves=6)) is None       # 16 >> 5 == 0
    for bad in (dict(sigma=0.0), dict(contrast_threshold=float("nan")), dict(edge_threshold=float("inf")), dict(n_octave_layers=0),
                dict(n_octave_layers=9), dict(border=0), dict(init_sigma=-0.5), dict(max_steps=0)):
        assert R.plan(64, 64, R.params(**bad)) is None, bad
    assert R.cv_round(2.5) == 2 and R.cv_round(3.5) == 4 and R.cv_round(-0.5) == 0
    assert R.threshold(p) == 1.0 and R.threshold(R.params(contrast_threshold=0.09)) == 3.0


def test_taps_are_symmetric_and_sum_to_one():
    for sig in (0.1, 0.7, 1.2262734984654078, 1.6, 3.0901, 5.9):
        t = R.taps(sig)
        assert len(t) == 2 * R.radius(sig) + 1 and t.dtype == np.float32
        assert np.array_equal(t, t[::-1]) and (t > 0).all() and t.argmax() == len(t) // 2
        s = 0.0
        for v in t:
            s += float(v)
        assert abs(s - 1.0) <= len(t) * 2.0 ** -24           # each tap is rounded once, by at most half a float ulp of a value < 1


def test_fold_matches_a_mirror_walk():
    def walk(i, n):
        if n == 1:
            return 0
        at, step = 0, 1
        for _ in range(abs(i)):
            if not 0 <= at + step < n:
                step = -step
            at += step
        return at

    for n in range(1, 9):
        i = np.arange(-40, 41 + n)
        assert R.fold(i, n).tolist() == [walk(int(k), n) for k in i], n


def test_blur_keeps_a_constant_and_a_single_pixel():
    t = R.taps(1.6)
    c = R.blur(np.full((4, 6), 100.0, np.float32), t)
    assert np.abs(c - 100.0).max() < 1e-4
    one = R.blur(np.full((1, 1), 7.0, np.float32), R.taps(3.0))
    assert one.shape == (1, 1) and abs(one[0, 0] - 7.0) < 1e-5


def test_a_constant_image_gives_no_candidate():
    p = R.params()
    for v in (0, 128, 255):
        kp, cand, _ = R.detect(np.full((37, 50), v, np.uint8), p)
        assert len(cand) == 0 and len(kp) == 0


def test_upsample_is_exact_and_clamped():
    img = S.ramp_image(7, 5)
    big = R.upsample2(img.astype(np.float32))
    assert big.shape == (10, 14) and big.dtype == np.float32
    assert big[0, 0] == img[0, 0] and big[-1, -1] == img[-1, -1]                            # clamped corners
    assert big[0, 1] == 0.75 * img[0, 0] + 0.25 * img[0, 1] and big[0, 2] == 0.25 * img[0, 0] + 0.75 * img[0, 1]
    assert np.array_equal(big * 16, np.rint(big * 16))       # multiples of 1/16


def test_an_isotropic_blob_scene_gives_one_keypoint_per_blob():
    p = R.params()
    kp, cand, why = R.detect(S.blob_image(), p)
    assert len(kp) == len(S.BLOBS) and len(cand) > len(kp)
    worst = 0.0
    for bx, by, sigma, _ in S.BLOBS:
        dist = np.hypot(kp["x"] - bx, kp["y"] - by)
        k = int(dist.argmin())
        worst = max(worst, float(dist[k]))
        # size is twice the keypoint's scale, and a Gaussian blob of deviation s answers the Laplacian at scale s: within 20 %
        # (the restatement shows 0.89 on all four: the difference of two Gaussians a factor 2^(1/3) apart sits below its finer scale)
        assert abs(kp["size"][k] / (2.0 * sigma) - 1.0) < 0.2, (sigma, kp["size"][k])
    print("largest distance to a blob's centre:", worst)
    assert worst <= BLOB_MAX_DISTANCE
    assert len({int(np.hypot(kp["x"] - bx, kp["y"] - by).argmin()) for bx, by, _, _ in S.BLOBS}) == len(S.BLOBS)


def test_pow2_is_within_two_ulp_of_exp2():
    e = np.linspace(0.0, 2.0, 100001).astype(np.float32)
    got, ref = R.pow2_frac(e), np.exp2(e.astype(np.float64))
    assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - ref) <= 2.0 * np.spacing(ref.astype(np.float32))).all()
    assert R.pow2_frac(np.float32([0.0, 1.0, 2.0])).tolist() == [1.0, 2.0, 4.0]


def test_solve3_pivots_and_rejects():
    A = np.float32([[[0, 0, 1], [0, 1, 0], [1, 0, 0]], [[1, 2, 3], [2, 4, 6], [1, 1, 1]], [[2, 0, 0], [0, 4, 0], [0, 0, 8]]])
    b = np.float32([[3, 2, 1], [1, 1, 1], [2, 4, 8]])
    x, zero = R.solve3(A, b)
    assert zero.tolist() == [False, True, False] and x[0].tolist() == [1, 2, 3] and x[2].tolist() == [1, 1, 1]


@pytest.mark.parametrize("over", [{}, {"n_octave_layers": 2, "border": 3}])
def test_the_generators_plant_what_they_say(over):
    p = R.params(**over)
    for f in (S.extrema_values, S.extrema_border, S.extrema_seams):
        d, want = f(70, 41, p)
        assert d.dtype == np.float32 and d.shape == (p.n_octave_layers + 2, 41, 70) and len(want) >= 4
    d, want = S.extrema_plateau(40, 30, p)
    assert len(want) == p.n_octave_layers * (40 - 2 * p.border) * (30 - 2 * p.border)


def test_the_refinement_stacks_meet_every_fate():
    p = R.params()
    d, cand, why = S.refine_walks(p)
    counts = S.assert_walks_cover(d, cand, why, p)
    assert counts[R.ZERO_PIVOT] == 0 and counts[R.TOO_FAR] == 0
    planted, sites = S.refine_planted(64, 24, p)
    S.assert_planted(planted, sites, p)
    kp, why2 = R.refine([d], cand, p)
    assert (np.abs(kp["xi"]) < 0.5).all() and (kp["response"] * 3 >= np.float32(0.04)).all() and (kp["layer"] >= 1).all() and (kp["layer"] <= 3).all()
    assert np.array_equal(why, why2)                         # the same call gives the same answer


def test_noise_image_keeps_hundreds_of_keypoints():
    kp, cand, why = R.detect(S.noise_image(), R.params())
    assert len(kp) > 100 and len(cand) > len(kp) and kp["octave"].max() >= 2
    order = np.lexsort((cand["col"], cand["row"], cand["layer"], cand["octave"]))
    assert np.array_equal(order, np.arange(len(cand)))       # ascending (octave, layer, row, col)

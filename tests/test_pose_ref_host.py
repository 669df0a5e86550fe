"""tests/poseref.py, the numpy restatement of the relative-pose recovery (include/lcm.h, lcm_pose_*), checked on its own,
and the pre-conditions of tests/test_gpu_pose.py checked with the reference alone: no GPU, no library."""
import numpy as np
import pytest

import epiref as E_
import posecases as S
import poseref as P


def test_decomposition_on_exact_integer_cases():
    """E = [t]x R with entries 0 and +-1: the scale is 1, every product and root is exact, so Ra is R itself, Rb is R turned
    half way about t or the other way round, and t comes back with the sign the cross products give it (the same for E and
    -E): Ra = R exactly when sign(E) x sign(t^) is +."""
    signs = []
    for E, R, t in S.integer_cases():
        for sign in (1.0, -1.0):
            ok, ra, rb, tt = P.decompose(sign * E)
            assert ok[0]
            twisted = (2.0 * np.outer(t, t) - np.eye(3)) @ R
            st = 1.0 if (tt[0] == t).all() else -1.0
            signs.append(st)
            np.testing.assert_array_equal(tt[0], st * t)
            first, second = (ra, rb) if sign * st > 0 else (rb, ra)
            np.testing.assert_array_equal(first[0].reshape(3, 3), R)
            np.testing.assert_array_equal(second[0].reshape(3, 3), twisted)
        R4, t4, status = P.candidates(E)
        assert status[0] == P.OK
        np.testing.assert_array_equal(R4[0, 2], R4[0, 0])
        np.testing.assert_array_equal(R4[0, 3], R4[0, 1])
        np.testing.assert_array_equal(t4[0, 2], -t4[0, 0])
        np.testing.assert_array_equal(t4[0, 1], t4[0, 0])
    assert signs[0::2] == signs[1::2] and set(signs) == {1.0, -1.0}          # no sign canonicalisation: both occur


def test_decomposition_of_random_motions():
    E = S.random_essentials(200, 3)
    ok, ra, rb, t = P.decompose(E)
    assert ok.all()
    for r in (ra, rb):
        r = r.reshape(-1, 3, 3)
        assert np.abs(r @ r.transpose(0, 2, 1) - np.eye(3)).max() < 1e-13
        assert np.abs(np.linalg.det(r) - 1.0).max() < 1e-13
    assert np.abs(np.linalg.norm(t, axis=1) - 1.0).max() < 1e-15
    rng = np.random.default_rng(3)                                  # the motions random_essentials drew, again
    for m in range(200):
        R = E_.rodrigues(rng.normal(0.0, 0.5, 3))
        tt = rng.normal(0.0, 1.0, 3)
        rng.choice([-1.0, 1.0]), rng.uniform(-3.0, 3.0)
        err = min(np.abs(ra[m].reshape(3, 3) - R).max(), np.abs(rb[m].reshape(3, 3) - R).max())
        assert err < 1e-13, (m, err)
        assert min(np.abs(t[m] - tt / np.linalg.norm(tt)).max(), np.abs(t[m] + tt / np.linalg.norm(tt)).max()) < 1e-13


def test_matrices_without_a_model():
    bad = np.array([np.zeros(9), [np.nan] + [0.0] * 8, [1e200, 0, 0, 0, 1e200, 0, 0, 0, 0], [1.0] + [0.0] * 8, [np.inf] + [1.0] * 8])
    R4, t4, status = P.candidates(bad)
    assert (status == P.NO_MODEL).all() and not R4.any() and not t4.any() and not np.signbit(t4).any()
    r = P.recover(np.zeros(9), np.zeros((5, 4), np.float32))
    assert (r["status"], r["choice"], r["n_used"], r["n_good"]) == (P.NO_MODEL, -1, 0, 0) and not r["mask"].any() and len(r["mask"]) == 5


def test_hand_checked_depth_verdicts():
    """Camera 2 one unit ahead of camera 1 along z (X2 = X1 + e_z under (I, e_z)) or one unit to the side (X2 = X1 + e_x)."""
    eye = np.eye(3).reshape(9)
    f = lambda r, t, x1, x2, md=50.0: bool(P.in_front(r, t, np.float64(x1[0]), np.float64(x1[1]), np.float64(x2[0]), np.float64(x2[1]), md))      # noqa: E731
    ez, ex = np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0])
    # X1 = (0.5, 0, 4), X2 = (0.5, 0, 5): in front of both; depths 4 and 5 baselines
    assert f(eye, ez, (0.125, 0.0), (0.1, 0.0))
    lam = P.depths(eye, ez, np.array([0.125]), np.array([0.0]), np.array([0.1]), np.array([0.0]))
    assert abs(lam[0][0] - 4.0) < 1e-12 and abs(lam[1][0] - 5.0) < 1e-12
    assert f(eye, ez, (0.125, 0.0), (0.1, 0.0), 5.0 + 1e-9) and not f(eye, ez, (0.125, 0.0), (0.1, 0.0), 5.0 - 1e-9)      # just inside / outside
    # sideways, X2 = X1 + e_x: X1 = (0, 0, 2) -> x2 = (0.5, 0); behind both: the rays meet at X1 = (0, 0, -2), x2 = (-0.5, 0)
    assert f(eye, ex, (0.0, 0.0), (0.5, 0.0))
    assert not f(eye, ex, (0.0, 0.0), (-0.5, 0.0))
    lam = P.depths(eye, ex, np.array([0.0]), np.array([0.0]), np.array([-0.5]), np.array([0.0]))
    assert lam[0][0] < 0 and lam[1][0] < 0
    # forward, X2 = X1 + e_z: X1 = (0.1, 0, -0.5) is behind the first camera only (X2 = (0.1, 0, 0.5)): x1 = (-0.2, 0), x2 = (0.2, 0)
    lam = P.depths(eye, ez, np.array([-0.2]), np.array([0.0]), np.array([0.2]), np.array([0.0]))
    assert lam[0][0] < 0 < lam[1][0] and not f(eye, ez, (-0.2, 0.0), (0.2, 0.0))
    # backward, X2 = X1 - e_z: X1 = (0.1, 0, 0.5) is behind the second camera only
    lam = P.depths(eye, -ez, np.array([0.2]), np.array([0.0]), np.array([-0.2]), np.array([0.0]))
    assert lam[1][0] < 0 < lam[0][0] and not f(eye, -ez, (0.2, 0.0), (-0.2, 0.0))
    # identical rays: D == 0, under any translation
    for t in (ez, -ez, ex):
        assert not f(eye, t, (0.25, -0.5), (0.25, -0.5))
    assert not f(eye, ez, (0.0, 0.0), (0.0, 0.0))


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_e_and_minus_e_give_the_same_pose(name):
    """The cofactor matrix and the cross products are even in E, [t]x E is odd: Ra and Rb change places and nothing else does.
    The chosen R, t, the mask, n_used and n_good are the same bytes; counts are the same numbers at k ^ 1."""
    pts, kind, E, *_ = S.scene(name)
    for mask in (None, S.planted_mask(kind)):
        p, m = P.recover(E, pts, mask), P.recover(-E, pts, mask)
        assert p["R"].tobytes() == m["R"].tobytes() and p["t"].tobytes() == m["t"].tobytes()
        assert p["mask"].tobytes() == m["mask"].tobytes() and (p["n_used"], p["n_good"]) == (m["n_used"], m["n_good"])
        assert m["choice"] == p["choice"] ^ 1 and list(m["counts"]) == [int(p["counts"][h ^ 1]) for h in range(4)]
        s = P.recover(3.7 * E, pts, mask)                               # another scale: the same verdicts
        assert s["choice"] == p["choice"] and s["mask"].tobytes() == p["mask"].tobytes()


def margin(counts):
    c = np.sort(np.asarray(counts))[::-1]
    return int(c[0] - c[1])


@pytest.mark.parametrize("name", ("forward", "sideways", "general", "twisted"))
def test_preconditions_of_the_planted_scenes(name):
    """With the reference alone: the winner leads by at least 10, the true motion is the chosen one, and the planted records the
    depth test refuses are those whose least-squares depth lies outside max_depth: counted, and at most 5 % of the planted."""
    pts, kind, E, R, t = S.scene(name)
    planted = kind != 2
    a, b, c, d = E_.normalise(pts)
    for mask in (None, S.planted_mask(kind)):
        for sign in (1.0, -1.0):
            r = P.recover(sign * E, pts, mask)
            assert r["status"] == P.OK and margin(r["counts"]) >= 10, (name, r["counts"])
            dR, dt = P.motion_error(r["R"], r["t"], R, t)
            assert dR <= S.TRUTH_TOL and dt <= S.TRUTH_TOL, (name, dR, dt)
            l1, l2 = P.depths(r["R"], r["t"], a, b, c, d)
            outside = planted & ~((l1 > 0) & (l2 > 0) & (l1 < P.MAX_DEPTH) & (l2 < P.MAX_DEPTH))
            assert 0 < outside.sum() <= 0.05 * planted.sum(), (name, outside.sum())
            np.testing.assert_array_equal(r["mask"][planted], (~outside[planted]).astype(np.uint8))
            assert outside[kind == 1].all() and not outside[kind == 0].any()           # exactly the far points
            assert r["n_used"] == (len(pts) if mask is None else planted.sum())
            assert r["n_good"] == r["mask"].sum() > P.MIN_POSE_INLIERS
            if mask is not None:
                assert not r["mask"][~planted].any()
    if name == "twisted":                                                              # the trap: the other rotation is the identity
        _, ra, rb, _ = P.decompose(E)
        other = rb if np.abs(ra[0].reshape(3, 3) - R).max() < 1e-12 else ra
        assert np.abs(other[0].reshape(3, 3) - np.eye(3)).max() < 1e-12


def test_preconditions_of_the_parity_cases():
    """Every (size, mask, max_depth) of the GPU parity test that uses at least 20 records has a winner that leads by 10: a
    last-bit difference cannot flip a choice there.  (One record, and no record, cannot lead by 10: those compare exactly or
    are the tie cases below.)"""
    pts, kind, E, R, t = S.scene("p1025")
    seen = 0
    for n in S.PARITY_SIZES:
        for mk in S.MASKS:
            for md in S.MAX_DEPTHS:
                r = P.recover(E, pts[:n], S.mask_of(mk, n), md)
                if r["n_used"] >= 20:
                    seen += 1
                    assert margin(r["counts"]) >= 10, (n, mk, md, r["counts"])
                    assert max(P.motion_error(r["R"], r["t"], R, t)) <= S.TRUTH_TOL
    assert seen >= 40
    full, cut = P.recover(E, pts, None, S.MAX_DEPTHS[0]), P.recover(E, pts, None, S.MAX_DEPTHS[1])
    assert cut["n_good"] < 0.8 * full["n_good"] and cut["n_good"] > 100           # the second limit does cut through the scene


def test_tie_cases_choose_the_first_hypothesis():
    pts, kind, E, *_ = S.scene("general")
    r = P.recover(E, pts, np.zeros(len(pts), np.uint8))
    assert (r["choice"], r["n_used"], r["n_good"], r["status"]) == (0, 0, 0, P.OK) and not r["counts"].any() and not r["mask"].any()
    Ez = P.essential(np.eye(3), [0.0, 0.0, 1.0])                           # Ra = I, Rb = diag(-1, -1, 1): (0, 0, 1) stays under both
    one = np.zeros((1, 4), np.float32)
    r = P.recover(Ez, one, None, 50.0, S.K_UNIT)
    assert (r["choice"], r["n_used"], r["n_good"]) == (0, 1, 0) and not r["counts"].any() and r["mask"].tolist() == [0]
    np.testing.assert_array_equal(r["R"].reshape(3, 3), np.eye(3))
    np.testing.assert_array_equal(r["t"], [0.0, 0.0, 1.0])


def test_many_pairs_case_is_worth_checking():
    pts, offs, E = S.many_pairs(2000)
    res, mask = P.recover_pairs(E, pts, offs)
    assert all(r["status"] == P.OK for r in res)
    good = np.array([r["n_good"] for r in res])
    assert (good >= 6).mean() > 0.04 and (good == 0).any() and len({r["choice"] for r in res}) == 4


def test_best_loop_walk():
    c = [(210, 300, 150, 0), (260, 300, 150, 0), (290, 300, 100, 0), (260, 300, 150, 0), (150, 300, 150, 0), (280, 300, 150, 1)]
    assert P.best_loop(c) == 1 and P.best_loop(c, 259) == 1 and P.best_loop(c, 260) == -1 and P.best_loop([]) == -1
    assert P.best_loop(c[2:3]) == -1 and P.best_loop(c[::-1]) == 2
    assert not P.pose_loop_test(250, 300, 100) and P.pose_loop_test(250, 300, 101) and not P.pose_loop_test(200, 300, 101)

"""tests/baref.py on its own, without a device: its float64 rounding over the very cases the GPU tests use (against np.longdouble
for r, J, H, g; route A, Cholesky, against route B, lstsq on [J; sqrt(damping) I], for one step's dp, the phases and whole runs
at min_update = 0).  The worst values measured here, rounded up, are the constants OWN_* of tests/bacases.py; the device gets
16 x those.  Also: (a) a literal transcription of the reference's sequential loops gives array_equal results with the
all-at-once phases; (b) every behavioural claim tests/test_gpu_ba.py makes about a case is shown of the restatement first."""
import numpy as np
import pytest

import bacases as S
import baref as B

LD = np.longdouble


def linearisations(m, dt):
    P = np.concatenate([B.G.log(m.R)[0], m.t], 1)
    rc, Jc = B.camera_linearise(m.K, P, m.X, m.cam, m.pt, m.uv, dt=dt)
    rp, Jp = B.point_linearise(m.K, m.R, m.t, m.X, m.cam, m.pt, m.uv, dt=dt)
    return (rc, Jc, m.cam, len(m.R)), (rp, Jp, m.pt, len(m.X))


def test_own_rounding_of_one_linearisation():
    worst = dict(r=0.0, J=0.0, H=0.0, g=0.0, cost=0.0)
    for name, build in S.STEP_CASES.items():
        m, _ = build()
        for (r, J, idx, n), (rl, Jl, _, _) in zip(linearisations(m, np.float64), linearisations(m, LD)):
            sr, sj = S.scales(r, J)
            worst["r"] = max(worst["r"], float(np.abs(r - rl).max()) / sr)
            worst["J"] = max(worst["J"], float(np.abs(J - Jl).max()) / sj)
            H, g, cost = B.normal(r, J, idx, n)
            Hl, gl, costl = B.normal(rl, Jl, idx, n)
            seen = np.bincount(idx, minlength=n) > 0
            scale_h, scale_g = np.abs(Hl).max((1, 2))[seen], np.abs(gl).max(1)[seen]
            worst["H"] = max(worst["H"], float((np.abs(H - Hl).max((1, 2))[seen] / scale_h).max()))
            worst["g"] = max(worst["g"], float((np.abs(g - gl).max(1)[seen] / np.maximum(scale_g, scale_h * 1e-6)).max()))
            worst["cost"] = max(worst["cost"], float((np.abs(cost - costl)[seen] / costl[seen]).max()))
    print("worst:", {k: f"{v:.3g}" for k, v in worst.items()}, "OWN_R", S.OWN_R, "OWN_J", S.OWN_J, "OWN_H_REL", S.OWN_H_REL)
    assert worst["r"] <= S.OWN_R and worst["J"] <= S.OWN_J
    assert worst["H"] <= S.OWN_H_REL and worst["g"] <= S.OWN_H_REL and worst["cost"] <= S.OWN_COST_REL
    assert S.OWN_R <= 4e-12 and S.OWN_J <= 4e-6                # no wider than the scale of the prototype's measurement


def refined(m, pp):
    """The elements a phase refines under pp: (cameras, points)."""
    cams = m.valid & (np.bincount(m.cam, minlength=len(m.R)) >= pp["min_cam_obs"]) & B.G.log(m.R)[1]
    return cams, np.bincount(m.pt, minlength=len(m.X)) >= pp["min_point_obs"]


def test_own_rounding_of_one_step():
    worst = 0.0
    pp = B.params({})
    for name, build in S.STEP_CASES.items():
        m, _ = build()
        for ((r, J, idx, n), todo) in zip(linearisations(m, np.float64), refined(m, pp)):
            a, ok_a, _, _, _ = B.solve("a", r, J, idx, n, pp["damping"])
            b, ok_b, _, _, _ = B.solve("b", r, J, idx, n, pp["damping"])
            assert ok_a[todo].all() and ok_b[todo].all(), name
            if todo.any():
                worst = max(worst, float(np.abs(a - b)[todo].max()))
    print(f"worst: A - B {worst:.3g} (OWN_DP {S.OWN_DP:.3g})")
    assert worst <= S.OWN_DP


def test_own_rounding_of_phases_and_runs():
    worst, worst_mean = 0.0, 0.0
    for name, build in S.RUN_CASES.items():
        m, _ = build()
        Ra, ta, ia = B.refine_cameras(m, "a", min_update=0.0)
        Rb, tb, ib = B.refine_cameras(m, "b", min_update=0.0)
        Xa, ja = B.refine_points(m, "a", min_update=0.0)
        Xb, jb = B.refine_points(m, "b", min_update=0.0)
        assert np.array_equal(ia["status"], ib["status"]) and np.array_equal(ia["iterations"], ib["iterations"]), name
        assert np.array_equal(ja["status"], jb["status"]) and np.array_equal(ja["iterations"], jb["iterations"]), name
        assert set(ia["iterations"]) <= {0, 5} and set(ja["iterations"]) <= {0, 5}             # every iteration runs: the counts are fixed
        worst = max(worst, float(np.abs(Ra - Rb).max()), float(np.abs(ta - tb).max()), float(np.abs(Xa - Xb).max()))
        a, _, _, ea = B.optimize(m, "a", min_update=0.0)
        b, _, _, eb = B.optimize(m, "b", min_update=0.0)
        worst = max(worst, float(np.abs(a.R - b.R).max()), float(np.abs(a.t - b.t).max()), float(np.abs(a.X - b.X).max()))
        worst_mean = max(worst_mean, float(np.abs(ea - eb).max()))
        assert ea[-1] < ea[0], name                                  # (b) the error falls on the planted scenes
    m = S.refine_map_case()
    (a, _, ra), (b, _, rb) = B.refine_map(m, "a", min_update=0.0), B.refine_map(m, "b", min_update=0.0)
    worst = max(worst, float(np.abs(a.R - b.R).max()), float(np.abs(a.t - b.t).max()), float(np.abs(a.X - b.X).max()))
    worst_mean = max([worst_mean] + [abs(ra[k] - rb[k]) for k in ("error_before", "error_after", "error_filtered", "error_final")])
    print(f"worst: entries {worst:.3g} (OWN_RUN {S.OWN_RUN:.3g}), mean errors {worst_mean:.3g} (OWN_MEAN {S.OWN_MEAN:.3g})")
    assert worst <= S.OWN_RUN and worst_mean <= S.OWN_MEAN


def test_the_sequential_loops_give_the_all_at_once_phases():
    """(a): one camera after another, one point after another, each scanning the whole list, against every element at once."""
    m, _ = S.planted(5, 24, 31, per_point=3, shuffle=True, invalid=(1,))
    m.R[3] = np.diag([-1.0, 1.0, -1.0])                               # a half turn: left alone by both
    for over in (dict(outer_iters=2, min_cam_obs=4), dict(outer_iters=2, min_cam_obs=4, min_update=0.0, inner_iters=3)):
        want = B.sequential(m, **over)
        got, ci, pi, _ = B.optimize(m, "a", **over)
        assert np.array_equal(got.R, want.R) and np.array_equal(got.t, want.t) and np.array_equal(got.X, want.X)
        assert ci["status"][1] == B.SKIPPED and ci["status"][3] == B.HALF_TURN and (ci["status"][[0, 2, 4]] < 2).all()
        assert not np.array_equal(got.R[0], m.R[0]) and np.array_equal(got.R[3], m.R[3]) and np.array_equal(got.R[1], m.R[1])


def test_the_planted_scene_behaves_as_the_prototype():
    """The issue's prototype: 12 cameras, 400 points, 0.5 px noise, fx = 1000: the mean error falls to the noise's level in five
    outer iterations; under the default min_update both kinds of element occur: converged before inner_iters and not."""
    m, _ = S.planted(12, 400, 1)
    a, ci, pi, means = B.optimize(m)
    print("mean errors", means)
    assert means[0] > 5.0 and means[-1] < 0.6 and (np.diff(means) < 0).all()


def test_both_kinds_of_element_occur_in_the_stop_rule_cases():
    """Under the default min_update: elements that stop before inner_iters updates, elements that stop at the last one and
    elements that never do, among the cameras and among the points."""
    cams, points = [], []
    for name, build in S.STOP_CASES.items():
        m, _ = build()
        cams.append(B.refine_cameras(m)[2])
        points.append(B.refine_points(m)[1])
    for info in (np.concatenate(cams), np.concatenate(points)):
        conv = info["status"] == B.CONVERGED
        assert conv.any() and (info["status"] == B.MAX_ITERS).any() and (info["iterations"][conv] < 5).any()
        assert (info["last_update"][conv] < 1e-6).all() and (info["last_update"][~conv] >= 1e-6).all()


def test_claims_about_the_special_cases():
    """(b): what tests/test_gpu_ba.py says of a case is true of the restatement."""
    pp = B.params({})
    # camera counts: below min_cam_obs skipped, at and above refined
    m, _ = S.camera_counts(S.CAMERA_COUNTS, 300, 3)
    _, _, ci = B.refine_cameras(m)
    assert [int(s == B.SKIPPED) for s in ci["status"]] == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert np.bincount(m.cam, minlength=10).tolist() == S.CAMERA_COUNTS
    # point counts: below min_point_obs skipped and byte for byte
    m, _ = S.point_counts(S.POINT_COUNTS, 20, 4)
    X, pi = B.refine_points(m)
    few = np.array(S.POINT_COUNTS) < 2
    assert ((pi["status"] == B.SKIPPED) == few).all() and np.array_equal(X[few], m.X[few]) and not (X[~few] == m.X[~few]).all(1).any()
    # a point seen twice by each of two cameras is refined
    m, _ = S.seen_twice(5)
    assert np.bincount(m.pt)[0] == 4 and set(m.cam[m.pt == 0]) == {0, 1}
    assert B.refine_points(m)[1]["status"][0] in (B.CONVERGED, B.MAX_ITERS)
    # an invalid camera is skipped and no observation names it
    m, _ = S.planted(12, 100, 6, invalid=(4,))
    assert not (m.cam == 4).any() and B.refine_cameras(m)[2]["status"][4] == B.SKIPPED
    # a point behind a camera: finite, the division goes on
    m, _ = S.behind(7)
    z = B.depths(m.R[m.cam], m.t[m.cam], m.X[m.pt])
    assert (z[m.pt == 7] < 0).any() and np.isfinite(B.refine_points(m)[0]).all() and np.isfinite(B.mean_error(m))
    # a depth of exactly 0: NaN, SOLVE_FAILED for the camera and for the point, both unchanged (the camera through exp(log R))
    m, _ = S.zero_depth(8)
    z = B.depths(m.R[m.cam], m.t[m.cam], m.X[m.pt])
    hit = (m.cam == 2) & (m.pt == 5)
    assert hit.sum() >= 1 and (z[hit] == 0).all()
    R, t, ci = B.refine_cameras(m)
    X, pi = B.refine_points(m)
    assert ci["status"][2] == B.SOLVE_FAILED and ci["iterations"][2] == 0 and not np.isfinite(ci["cost"][2])
    assert np.array_equal(R[2], np.eye(3)) and np.array_equal(t[2], m.t[2])
    assert pi["status"][5] == B.SOLVE_FAILED and pi["iterations"][5] == 0 and np.array_equal(X[5], m.X[5])
    assert (np.delete(ci["status"], 2) != B.SOLVE_FAILED).all() and (np.delete(pi["status"], 5) != B.SOLVE_FAILED).all()
    # a half-turn camera
    m, _ = S.half_turn(9)
    R, t, ci = B.refine_cameras(m)
    assert ci["status"][3] == B.HALF_TURN and np.array_equal(R[3], m.R[3]) and (np.delete(ci["status"], 3) < 2).all()
    # the whole run under the defaults on the scene with an invalid camera: from above 5 px to below 0.6 px
    means = B.optimize(S.planted(12, 100, 6, invalid=(4,))[0])[3]
    assert means[-1] < 0.6 < 5.0 < means[0]
    # cameras with exactly ten observations are refined
    assert (B.refine_cameras(S.camera_counts([10] * 65, 200, 14)[0], min_update=0.0, inner_iters=2)[2]["status"] == B.MAX_ITERS).all()


def test_the_outlier_cases_stand_clear_of_every_threshold():
    m, planted = S.outlier_scene()
    flags, worst, thr, look = B.outliers(m)
    assert set(np.flatnonzero(flags)) == planted
    assert not ((look["err"] >= 4.9) & (look["err"] <= 5.1)).any() and not (np.abs(look["depth"]) <= 1e-6).any()
    assert not (np.abs(look["dist"] - thr) <= 1e-6 * thr).any() and thr > 10.0
    assert (look["depth"] <= 0).sum() >= 2 and (look["err"][look["depth"] > 0] > 5.0).sum() >= 2 and (look["dist"] > thr).sum() == 2
    ok = np.ones(len(m.X), bool)
    ok[list(planted)] = False
    assert (worst[ok] < 1.0).all() and worst[3] >= 20.0
    # lcm_ba_refine_map's case: after the first adjustment nothing lies within 1e-3 px of outlier_px (min_update = 0: the GPU test's setting)
    m = S.refine_map_case()
    final, table, rep = B.refine_map(m, min_update=0.0)
    err, depth = rep["look"]["err"], rep["look"]["depth"]
    assert np.abs(err - 5.0).min() > 1e-3 and 1e-3 > 16 * S.OWN_RUN * 4e3 and 1e-3 > 16 * S.OWN_MEAN and np.abs(depth).min() > 1e-3
    assert np.abs(rep["look"]["dist"] - rep["threshold"]).min() > 1e-3
    assert rep["n_outliers"] >= 4 and (table[[5, 50, 120, 170]] == -1).all() and rep["n_points"] == 200 - rep["n_outliers"]
    assert rep["error_final"] < rep["error_filtered"] < rep["error_after"] < rep["error_before"] and rep["error_final"] < 0.6
    # route B agrees on the flags and on the run
    final_b, table_b, rep_b = B.refine_map(m, "b", min_update=0.0)
    assert np.array_equal(table, table_b) and np.abs(final.X - final_b.X).max() <= S.OWN_RUN


def test_compaction_and_loop_observations():
    m, _ = S.planted(6, 30, 41, per_point=3, shuffle=True)
    flags = (np.arange(30) % 4 == 1).astype(np.uint8)
    c, table = B.compact(m, flags)
    # a walk of :1633-1659
    old_to_new, pts, obs = [-1] * 30, [], []
    for i in range(30):
        if not flags[i]:
            old_to_new[i] = len(pts)
            pts.append(m.X[i])
    for i in range(len(m.cam)):
        if old_to_new[m.pt[i]] != -1:
            obs.append((m.cam[i], old_to_new[m.pt[i]], m.uv[i, 0], m.uv[i, 1]))
    assert table.tolist() == old_to_new and np.array_equal(c.X, np.array(pts))
    assert [(a, b, u, v) for a, b, (u, v) in zip(c.cam, c.pt, c.uv)] == obs
    matches, mask, past, curr, kp, n_points = S.loop_lists()
    new, table = B.add_loop_observations(matches, mask, past, curr, kp, 9)
    assert 5 < len(new) < mask.sum() and all(c == 9 and 0 <= p < n_points for c, p, _, _ in new)
    assert (table != curr).sum() > 0 and (table[curr == 7] != -1).all()

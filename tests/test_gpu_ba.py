"""The alternating bundle adjustment and the outlier removal on the device (include/lcm.h lcm_ba_*; lcm_ba.hip, lcm_ba.cpp) against
tests/baref.py.  Needs a real MI355X.

Accuracy is compared at min_update = 0, where every iteration runs and the counts are fixed, within 16 x the restatement's own
float64 rounding (tests/bacases.py OWN_*, measured by tests/test_ba_ref_host.py over the same cases).  The stop rule is checked on
the device's own bytes: the runs with inner_iters = 1 .. 5 at min_update = 0 are prefixes of one trajectory, and the default run
must return, per element, the record of the first prefix whose last_update < min_update.  Outlier flags are compared exactly."""
import ctypes as C

import numpy as np
import pytest

import bacases as S
import baref as B
import epiref as E_

pytestmark = pytest.mark.gpu

FILL = 0xA7
M = S.MARGIN
_cache = {}


def case(table, name):
    """A case's map, built once and never changed."""
    key = (id(table), name)
    if key not in _cache:
        _cache[key] = table[name]()[0]
    return _cache[key]


def records(pkg, m):
    c = pkg.capi
    return c.pgo_poses(m.R, m.t), c.ba_points(m.X), c.ba_obs(m.cam, m.pt, m.uv), m.valid.astype(np.uint8)


def bp(pkg, m=None, **over):
    K = S.K if m is None else m.K
    return pkg.capi.default_ba_params(**{**dict(fx=K[0], fy=K[1], cx=K[2], cy=K[3]), **over})


def as_bytes(a):
    return np.ascontiguousarray(a).tobytes()


def refined(m, pp):
    cams = m.valid & (np.bincount(m.cam, minlength=len(m.R)) >= pp["min_cam_obs"]) & B.G.log(m.R)[1]
    return cams, np.bincount(m.pt, minlength=len(m.X)) >= pp["min_point_obs"]


def check_step(name, got, r, J, idx, n, todo, damping):
    gr, gJ, gH, gg, gdp, ginfo = got
    sr, sj = S.scales(r[todo[idx]], J[todo[idx]]) if todo[idx].any() else (1.0, 1.0)
    of = todo[idx]
    err_r, err_j = np.abs(gr - r)[of].max(initial=0.0), np.abs(gJ - J)[of].max(initial=0.0)
    assert not gr[~of].any() and not gJ[~of].any(), name                      # an element that is not linearised: zeros
    dp, ok, H, g, cost = B.solve("a", r, J, idx, n, damping)
    scale_h = np.abs(H).max((1, 2))
    err_h = (np.abs(gH - H).max((1, 2))[todo] / scale_h[todo]).max(initial=0.0)
    err_g = (np.abs(gg - g).max(1)[todo] / np.maximum(np.abs(g).max(1), scale_h * 1e-6)[todo]).max(initial=0.0)
    # the closure on the device's own output: route A on ITS r and J (OWN_DP is two solves of one linearisation)
    gr_own, gJ_own = np.where(of[:, None], gr, r), np.where(of[:, None, None], gJ, J)
    err_dp = np.abs(gdp - B.solve("a", gr_own, gJ_own, idx, n, damping)[0])[todo].max(initial=0.0)
    err_c = (np.abs(ginfo["cost"] - cost)[todo] / cost[todo]).max(initial=0.0)
    print(f"{name}: r {err_r:.3g} J {err_j:.3g} H {err_h:.3g} g {err_g:.3g} dp {err_dp:.3g} cost {err_c:.3g}")
    assert err_r <= M * S.OWN_R * sr and err_j <= M * S.OWN_J * sj, name
    assert err_h <= M * S.OWN_H_REL and err_g <= M * S.OWN_H_REL and err_c <= M * S.OWN_COST_REL, name
    assert err_dp <= M * S.OWN_DP * max(sr, sj), name
    assert np.array_equal(gH, gH.transpose(0, 2, 1)) and not gH[~todo].any() and not gg[~todo].any() and not gdp[~todo].any()
    assert (ginfo["status"][~todo] >= B.HALF_TURN).all() and (ginfo["iterations"][todo] == 1).all() and ok[todo].all()
    assert np.array_equal(ginfo["last_update"][todo], np.abs(gdp).max(1)[todo])


@pytest.mark.parametrize("name", list(S.STEP_CASES))
def test_one_linearisation(pkg, matcher, name):
    m = case(S.STEP_CASES, name)
    poses, points, obs, valid = records(pkg, m)
    pp = B.params({})
    cams, pts = refined(m, pp)
    P = np.concatenate([B.G.log(m.R)[0], m.t], 1)
    r, J = B.camera_linearise(m.K, P, m.X, m.cam, m.pt, m.uv)
    check_step(name + " cameras", matcher.ba_step_cameras(poses, points, obs, bp(pkg), valid=valid), r, J, m.cam, len(m.R), cams, pp["damping"])
    r, J = B.point_linearise(m.K, m.R, m.t, m.X, m.cam, m.pt, m.uv)
    check_step(name + " points", matcher.ba_step_points(poses, points, obs, bp(pkg), valid=valid), r, J, m.pt, len(m.X), pts, pp["damping"])
    # the mean error and every observation's
    mean, each = matcher.ba_error(poses, points, obs, bp(pkg), valid=valid, per_observation=True)
    want = B.observation_errors(m)
    sr = max(1.0, float(want.max()) / 32)
    assert np.abs(each - want).max() <= M * S.OWN_R * sr and abs(mean - B.mean_error(m)) <= M * S.OWN_R * sr
    assert matcher.ba_error(poses, points, obs, bp(pkg), valid=valid) == mean


def check_infos(got, want, name):
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["iterations"], want["iterations"]), name
    ran = want["status"] < B.HALF_TURN
    assert np.abs(got["last_update"] - want["last_update"]).max(initial=0.0) <= M * S.OWN_RUN, name
    assert (np.abs(got["cost"] - want["cost"])[ran] <= 1e-6 * want["cost"][ran] + 1e-9).all(), name
    assert not got["cost"][~ran].any() and not got["last_update"][~ran].any()


@pytest.mark.parametrize("name", list(S.RUN_CASES))
def test_phases_and_whole_runs_at_min_update_zero(pkg, matcher, name):
    c = pkg.capi
    m = case(S.RUN_CASES, name)
    poses, points, obs, valid = records(pkg, m)
    p0 = bp(pkg, min_update=0.0)
    R, t, ci = B.refine_cameras(m, min_update=0.0)
    gp, gi = matcher.ba_refine_cameras(poses, points, obs, p0, valid=valid)
    err = max(np.abs(gp["R"].reshape(-1, 3, 3) - R).max(), np.abs(gp["t"] - t).max())
    check_infos(gi, ci, name)
    skipped = ci["status"] == B.SKIPPED
    assert as_bytes(gp[skipped]) == as_bytes(poses[skipped])
    X, pi = B.refine_points(m, min_update=0.0)
    gx, gj = matcher.ba_refine_points(poses, points, obs, p0, valid=valid)
    err = max(err, np.abs(c.ba_xyz(gx) - X).max())
    check_infos(gj, pi, name)
    assert as_bytes(gx[pi["status"] == B.SKIPPED]) == as_bytes(points[pi["status"] == B.SKIPPED])
    want, wci, wpi, means = B.optimize(m, min_update=0.0)
    op, ox, oci, opi, info = matcher.ba_optimize(poses, points, obs, p0, valid=valid)
    err_run = max(np.abs(op["R"].reshape(-1, 3, 3) - want.R).max(), np.abs(op["t"] - want.t).max(), np.abs(c.ba_xyz(ox) - want.X).max())
    err_mean = np.abs(np.array(info.mean_error[:6]) - means).max()
    print(f"{name}: phases {err:.3g}, run {err_run:.3g}, mean errors {err_mean:.3g}; {list(info.mean_error[:6])}")
    assert err <= M * S.OWN_RUN and err_run <= M * S.OWN_RUN and err_mean <= M * S.OWN_MEAN
    check_infos(oci, wci, name), check_infos(opi, wpi, name)
    assert info.outer_iters == 5 and not any(info.mean_error[6:]) and info.mean_error[5] < info.mean_error[0]
    assert list(info.cameras) == np.bincount(wci["status"], minlength=5).tolist() and list(info.points) == np.bincount(wpi["status"], minlength=5).tolist()


def test_the_stop_rule_on_the_devices_own_bytes(pkg, matcher):
    kinds = set()
    for name in S.STOP_CASES:
        m = case(S.STOP_CASES, name)
        poses, points, obs, valid = records(pkg, m)
        for cams, phase, inputs in ((True, matcher.ba_refine_cameras, poses), (False, matcher.ba_refine_points, points)):
            prefix = [phase(poses, points, obs, bp(pkg, min_update=0.0, inner_iters=k)) for k in range(1, 6)]
            out, info = phase(poses, points, obs, bp(pkg))
            for e in range(len(inputs)):
                if info["status"][e] == B.SKIPPED:
                    assert as_bytes(out[e]) == as_bytes(inputs[e])
                    continue
                first = next((k for k in range(5) if prefix[k][1]["last_update"][e] < 1e-6), 4)
                stopped = bool(prefix[first][1]["last_update"][e] < 1e-6)
                assert as_bytes(out[e]) == as_bytes(prefix[first][0][e]), (name, cams, e)
                w = prefix[first][1][e]
                assert (info["last_update"][e], info["cost"][e], info["iterations"][e]) == (w["last_update"], w["cost"], first + 1)
                assert info["status"][e] == (B.CONVERGED if stopped else B.MAX_ITERS)
                kinds.add((cams, stopped, first < 4))
    print(sorted(kinds))
    for cams in (True, False):                        # both phases have elements that stop early and elements that never stop
        assert {(cams, True, True), (cams, False, False)} <= kinds, kinds


def test_a_whole_run_under_the_defaults_keeps_its_invariants(pkg, matcher):
    m = case(S.STEP_CASES, "invalid")
    poses, points, obs, valid = records(pkg, m)
    p = bp(pkg)
    op, ox, ci, pi, info = matcher.ba_optimize(poses, points, obs, p, valid=valid)
    for inf in (ci, pi):
        conv, limit = inf["status"] == B.CONVERGED, inf["status"] == B.MAX_ITERS
        assert (inf["last_update"][conv] < 1e-6).all() and (inf["last_update"][limit] >= 1e-6).all() and (inf["iterations"] <= 5).all()
        assert (inf["iterations"][limit] == 5).all() and (conv | limit | (inf["status"] == B.SKIPPED)).all()
    assert ci["status"][4] == B.SKIPPED and as_bytes(op[4]) == as_bytes(poses[4])
    assert info.mean_error[0] == matcher.ba_error(poses, points, obs, p, valid=valid)
    assert info.mean_error[5] == matcher.ba_error(op, ox, obs, p, valid=valid)
    assert info.mean_error[5] < 0.6 < 5.0 < info.mean_error[0]
    assert list(info.cameras) == np.bincount(ci["status"], minlength=5).tolist() and list(info.points) == np.bincount(pi["status"], minlength=5).tolist()
    # a short run, and outputs written over the inputs
    p2 = bp(pkg, outer_iters=2)
    a = matcher.ba_optimize(poses, points, obs, p2, valid=valid)
    assert a[4].outer_iters == 2 and a[4].mean_error[2] > 0 and not any(a[4].mean_error[3:]) and a[4].mean_error[:2] == info.mean_error[:2]
    lib, pc, xc, ninfo = pkg.load_library(), poses.copy(), points.copy(), pkg.capi.BaInfo()
    rc = lib.lcm_ba_optimize(matcher._h, pc.ctypes.data, valid.ctypes.data, len(pc), xc.ctypes.data, len(xc), obs.ctypes.data, len(obs), C.byref(p2),
                             pc.ctypes.data, xc.ctypes.data, None, None, C.byref(ninfo))
    assert rc == 0 and as_bytes(pc) == as_bytes(a[0]) and as_bytes(xc) == as_bytes(a[1]) and bytes(ninfo) == bytes(a[4])


def test_special_cameras_and_points(pkg, matcher):
    c = pkg.capi
    # a half-turn camera: byte for byte, the others refined
    m, _ = S.half_turn(9)
    poses, points, obs, valid = records(pkg, m)
    gp, gi = matcher.ba_refine_cameras(poses, points, obs, bp(pkg))
    assert gi["status"][3] == B.HALF_TURN and as_bytes(gp[3]) == as_bytes(poses[3]) and (np.delete(gi["status"], 3) < 2).all()
    assert gi["iterations"][3] == 0 and gi["cost"][3] == 0
    _, _, ci, _, info = matcher.ba_optimize(poses, points, obs, bp(pkg))
    assert ci["status"][3] == B.HALF_TURN and info.cameras[B.HALF_TURN] == 1
    # a depth of exactly 0: SOLVE_FAILED before any update; the point unchanged, the camera as exp(log R)
    m, _ = S.zero_depth(8)
    poses, points, obs, valid = records(pkg, m)
    gp, gi = matcher.ba_refine_cameras(poses, points, obs, bp(pkg))
    gx, gj = matcher.ba_refine_points(poses, points, obs, bp(pkg))
    assert (gi["status"][2], gi["iterations"][2], gi["last_update"][2]) == (B.SOLVE_FAILED, 0, 0.0) and not np.isfinite(gi["cost"][2])
    assert as_bytes(gp[2]) == as_bytes(poses[2])                       # the identity pose: exp(log I) = I, t as it was
    assert (gj["status"][5], gj["iterations"][5]) == (B.SOLVE_FAILED, 0) and as_bytes(gx[5]) == as_bytes(points[5])
    assert (np.delete(gi["status"], 2) < 2).all() and (np.delete(gj["status"], 5) < 2).all()
    # a failed camera that is not the identity comes back as exp(log R): a rotation within rounding of the given one
    m.R[2] = B.G.exp(np.array([0.0, 0.0, 0.3]))
    poses = c.pgo_poses(m.R, m.t)
    gp, gi = matcher.ba_refine_cameras(poses, points, obs, bp(pkg))
    assert gi["status"][2] == B.SOLVE_FAILED
    assert np.abs(gp["R"][2] - poses["R"][2]).max() < 1e-15 and as_bytes(gp["t"][2]) == as_bytes(poses["t"][2])


def big_camera():
    """One camera with 70 000 observations (above 2^16; 20 000 points, so every point is seen several times by it), one with 300."""
    if "big" not in _cache:
        _cache["big"] = S.camera_counts([70000, 300], 20000, 12)[0]
    return _cache["big"]


def test_a_camera_with_70000_observations(pkg, matcher):
    m = big_camera()
    poses, points, obs, valid = records(pkg, m)
    P = np.concatenate([B.G.log(m.R)[0], m.t], 1)
    r, J = B.camera_linearise(m.K, P, m.X, m.cam, m.pt, m.uv)
    check_step("70000", matcher.ba_step_cameras(poses, points, obs, bp(pkg)), r, J, m.cam, 2, np.array([True, True]), 1e-3)
    R, t, ci = B.refine_cameras(m, min_update=0.0)
    gp, gi = matcher.ba_refine_cameras(poses, points, obs, bp(pkg, min_update=0.0))
    assert max(np.abs(gp["R"].reshape(-1, 3, 3) - R).max(), np.abs(gp["t"] - t).max()) <= M * S.OWN_RUN
    check_infos(gi, ci, "70000")


@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 257, 100003])
def test_point_counts(pkg, matcher, n_points):
    m, _ = S.planted(12, n_points, 13, per_point=3)
    poses, points, obs, valid = records(pkg, m)
    iters = 2 if n_points > 1000 else 5                                # the restatement's time at 300 009 observations
    X, pi = B.refine_points(m, min_update=0.0, inner_iters=iters)
    gx, gj = matcher.ba_refine_points(poses, points, obs, bp(pkg, min_update=0.0, inner_iters=iters))
    assert np.abs(pkg.capi.ba_xyz(gx) - X).max() <= M * S.OWN_RUN
    check_infos(gj, pi, str(n_points))
    flags, worst, thr, n = matcher.ba_outliers(poses, points, obs, bp(pkg))
    wf, ww, wthr, _ = B.outliers(m)
    assert abs(thr - wthr) <= 1e-12 and n == flags.sum() and np.abs(worst - ww).max() <= M * S.OWN_R * max(1.0, ww.max() / 32)
    assert abs(matcher.ba_error(poses, points, obs, bp(pkg)) - B.mean_error(m)) <= M * S.OWN_R * max(1.0, ww.max() / 32)


@pytest.mark.parametrize("n_cams", [1, 2, 65, 4096])
def test_camera_counts(pkg, matcher, n_cams):
    m, _ = S.camera_counts([10] * n_cams, 200, 14)
    poses, points, obs, valid = records(pkg, m)
    R, t, ci = B.refine_cameras(m, min_update=0.0, inner_iters=2)
    gp, gi = matcher.ba_refine_cameras(poses, points, obs, bp(pkg, min_update=0.0, inner_iters=2))
    assert (gi["status"] == B.MAX_ITERS).all() and (gi["iterations"] == 2).all()
    assert max(np.abs(gp["R"].reshape(-1, 3, 3) - R).max(), np.abs(gp["t"] - t).max()) <= M * S.OWN_RUN
    check_infos(gi, ci, str(n_cams))


def test_the_same_call_gives_the_same_bytes(pkg, matcher):
    m, other = case(S.STEP_CASES, "camera_counts"), case(S.STEP_CASES, "c65_p257")
    poses, points, obs, valid = records(pkg, m)
    first = matcher.ba_optimize(poses, points, obs, bp(pkg))
    step = matcher.ba_step_cameras(poses, points, obs, bp(pkg))
    matcher.ba_optimize(*records(pkg, other)[:3], bp(pkg))
    matcher.ba_step_points(*records(pkg, other)[:3], bp(pkg))
    again = matcher.ba_optimize(poses, points, obs, bp(pkg))
    step2 = matcher.ba_step_cameras(poses, points, obs, bp(pkg))
    assert all(as_bytes(a) == as_bytes(b) for a, b in zip(first[:4], again[:4])) and bytes(first[4]) == bytes(again[4])
    assert all(as_bytes(a) == as_bytes(b) for a, b in zip(step, step2))
    big = big_camera()
    rec = records(pkg, big)
    a, b = matcher.ba_refine_cameras(*rec[:3], bp(pkg)), matcher.ba_refine_cameras(*rec[:3], bp(pkg))
    assert as_bytes(a[0]) == as_bytes(b[0]) and as_bytes(a[1]) == as_bytes(b[1])


def test_outlier_flags_are_exact(pkg, matcher):
    m, planted = S.outlier_scene()
    poses, points, obs, valid = records(pkg, m)
    flags, worst, thr, n = matcher.ba_outliers(poses, points, obs, bp(pkg))
    wf, ww, wthr, _ = B.outliers(m)
    assert np.array_equal(flags, wf) and set(np.flatnonzero(flags)) == planted and n == len(planted)
    assert abs(thr - wthr) <= 1e-12 * wthr and np.abs(worst - ww).max() <= M * S.OWN_R * max(1.0, ww.max() / 32)
    # other thresholds
    flags2, _, thr2, n2 = matcher.ba_outliers(poses, points, obs, bp(pkg, outlier_px=100.0, min_spread=1000.0))
    assert thr2 == 1000.0 and np.array_equal(flags2, B.outliers(m, outlier_px=100.0, min_spread=1000.0)[0]) and n2 < n
    kept_x, kept_o, table = pkg.capi.ba_compact(points, obs, flags)
    cm, wt = B.compact(m, wf)
    assert np.array_equal(table, wt) and np.array_equal(pkg.capi.ba_xyz(kept_x), cm.X) and np.array_equal(kept_o["point"], cm.pt)


def test_refine_map_end_to_end(pkg, matcher):
    c = pkg.capi
    m = S.refine_map_case()
    poses, points, obs, valid = records(pkg, m)
    want, wtable, rep = B.refine_map(m, min_update=0.0)
    gp, gx, go, table, got = matcher.ba_refine_map(poses, points, obs, bp(pkg, min_update=0.0))
    assert np.array_equal(table, wtable) and (got.n_outliers, got.n_points, got.n_obs) == (rep["n_outliers"], rep["n_points"], rep["n_obs"])
    assert np.array_equal(go["cam"], want.cam) and np.array_equal(go["point"], want.pt) and np.array_equal(go["u"], want.uv[:, 0])
    err = max(np.abs(gp["R"].reshape(-1, 3, 3) - want.R).max(), np.abs(gp["t"] - want.t).max(), np.abs(c.ba_xyz(gx) - want.X).max())
    errs = [abs(getattr(got, k) - rep[k]) for k in ("error_before", "error_after", "error_filtered", "error_final")]
    print(f"refine_map: entries {err:.3g}, errors {max(errs):.3g}; {got.error_before:.4g} -> {got.error_after:.4g} -> {got.error_filtered:.4g} -> {got.error_final:.4g}")
    assert err <= M * S.OWN_RUN and max(errs) <= M * S.OWN_MEAN and abs(got.threshold - rep["threshold"]) <= 1e-9
    assert got.error_final < got.error_filtered < got.error_after < got.error_before
    # it is its steps
    p = bp(pkg, min_update=0.0)
    a = matcher.ba_optimize(poses, points, obs, p)
    flags, _, thr, n = matcher.ba_outliers(a[0], a[1], obs, p)
    kx, ko, t2 = c.ba_compact(a[1], obs, flags)
    b = matcher.ba_optimize(a[0], kx, ko, bp(pkg, min_update=0.0, outer_iters=3))
    assert as_bytes(b[0]) == as_bytes(gp) and as_bytes(b[1]) == as_bytes(gx) and as_bytes(ko) == as_bytes(go) and np.array_equal(t2, table)
    assert (got.error_before, got.error_after, got.error_filtered, got.error_final) == (a[4].mean_error[0], a[4].mean_error[5], b[4].mean_error[0], b[4].mean_error[3])
    assert (thr, n) == (got.threshold, got.n_outliers)


def test_launch_info(pkg, matcher):
    m = case(S.STEP_CASES, "shuffled")
    poses, points, obs, valid = records(pkg, m)
    matcher.ba_optimize(poses, points, obs, bp(pkg))
    info = matcher.launch_info()
    assert (info.launches, info.pairs) == (2 + 4 * 5, len(obs)) and info.kernel_ms > 0
    matcher.ba_optimize(poses, points, obs, bp(pkg, outer_iters=2))
    assert matcher.launch_info().launches == 10
    for call, launches in ((matcher.ba_refine_cameras, 1), (matcher.ba_refine_points, 1), (matcher.ba_step_cameras, 1), (matcher.ba_error, 2),
                           (matcher.ba_outliers, 1)):
        call(poses, points, obs, bp(pkg))
        info = matcher.launch_info()
        assert (info.launches, info.pairs) == (launches, len(obs)) and info.kernel_ms > 0
    # no observation at all: a mean of 0.0, every element skipped
    empty = obs[:0]
    assert matcher.ba_error(poses, points, empty, bp(pkg)) == 0.0
    gp, gx, ci, pi, info = matcher.ba_optimize(poses, points, empty, bp(pkg))
    assert as_bytes(gp) == as_bytes(poses) and as_bytes(gx) == as_bytes(points) and (ci["status"] == B.SKIPPED).all() and not any(info.mean_error)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def raw(pkg, matcher, name, poses, valid, points, obs, p, n=None, null=()):
    """One raw call with poisoned outputs: (status, whether every output is untouched)."""
    lib = pkg.load_library()
    n_poses, n_points, n_obs = n or (len(poses), len(points), len(obs))
    NC, NP, NO = (n_poses if poses is None else len(poses)), (n_points if points is None else len(points)), (n_obs if obs is None else max(len(obs), 1))
    sizes = {"lcm_ba_error": [8, 8 * NO], "lcm_ba_refine_cameras": [96 * NC, 24 * NC], "lcm_ba_refine_points": [24 * NP, 24 * NP],
             "lcm_ba_step_cameras": [16 * NO, 96 * NO, 288 * NC, 48 * NC, 48 * NC, 24 * NC],
             "lcm_ba_step_points": [16 * NO, 48 * NO, 72 * NP, 24 * NP, 24 * NP, 24 * NP],
             "lcm_ba_optimize": [96 * NC, 24 * NP, 24 * NC, 24 * NP, 184], "lcm_ba_outliers": [NP, 8 * NP, 8, 4],
             "lcm_ba_refine_map": [96 * NC, 24 * NP, 24 * NO, 4 * NP, 56]}[name]
    bufs = [np.full(s, FILL, np.uint8) for s in sizes]
    ptrs = [None if k in null else b.ctypes.data for k, b in enumerate(bufs)]
    if name == "lcm_ba_error":
        ptrs[0] = None if 0 in null else C.cast(bufs[0].ctypes.data, C.POINTER(C.c_double))
    if name == "lcm_ba_optimize":
        ptrs[4] = None if 4 in null else C.cast(bufs[4].ctypes.data, C.POINTER(pkg.capi.BaInfo))
    if name == "lcm_ba_outliers":
        ptrs[2], ptrs[3] = C.cast(bufs[2].ctypes.data, C.POINTER(C.c_double)), None if 3 in null else C.cast(bufs[3].ctypes.data, C.POINTER(C.c_int32))
    if name == "lcm_ba_refine_map":
        ptrs[4] = None if 4 in null else C.cast(bufs[4].ctypes.data, C.POINTER(pkg.capi.BaMapReport))
        ptrs = [0] + ptrs
    rc = getattr(lib, name)(matcher._h, None if poses is None else poses.ctypes.data, None if valid is None else valid.ctypes.data, n_poses,
                            None if points is None else points.ctypes.data, n_points, None if obs is None else obs.ctypes.data, n_obs,
                            None if p is None else C.byref(p), *ptrs)
    return rc, all((b == FILL).all() for b in bufs)


CALLS = ("lcm_ba_error", "lcm_ba_refine_cameras", "lcm_ba_refine_points", "lcm_ba_step_cameras", "lcm_ba_step_points", "lcm_ba_optimize",
         "lcm_ba_outliers", "lcm_ba_refine_map")


def test_refusals_write_nothing_and_leave_the_handle_usable(pkg, matcher):
    m = case(S.STEP_CASES, "invalid")
    poses, points, obs, valid = records(pkg, m)
    good = bp(pkg)
    before = matcher.ba_optimize(poses, points, obs, good, valid=valid)

    def changed(arr, index, field, value):
        out = arr.copy()
        out[field][index] = value
        return out

    stretched = poses.copy()
    stretched["R"][1] *= 1.001
    mirrored = poses.copy()
    mirrored["R"][1][:3] *= -1
    bad_inputs = [
        (None, valid, points, obs, good), (poses, valid, None, obs, good), (poses, valid, points, None, good), (poses, valid, points, obs, None),
        (poses, valid, points, changed(obs, 7, "cam", 12), good), (poses, valid, points, changed(obs, 7, "cam", -1), good),
        (poses, valid, points, changed(obs, 7, "point", len(points)), good), (poses, valid, points, changed(obs, 7, "point", -1), good),
        (poses, valid, points, changed(obs, 7, "cam", 4), good),                                     # an observation of an invalid camera
        (changed(poses, 1, "t", np.nan), valid, points, obs, good), (changed(poses, 0, "R", np.inf), valid, points, obs, good),
        (poses, valid, changed(points, 3, "y", np.inf), obs, good), (poses, valid, points, changed(obs, 9, "u", np.nan), good),
        (stretched, valid, points, obs, good), (mirrored, valid, points, obs, good),
    ]
    for field, value in (("fx", 0.0), ("fy", -1.0), ("fx", np.nan), ("cx", np.inf), ("eps", 0.0), ("damping", -1.0), ("min_update", np.nan),
                         ("outlier_px", -1.0), ("min_spread", np.inf), ("spread_factor", -1.0), ("outer_iters", 0), ("outer_iters", 17),
                         ("inner_iters", 0), ("inner_iters", 17), ("min_cam_obs", -1), ("min_point_obs", -1)):
        bad_inputs.append((poses, valid, points, obs, bp(pkg, **{field: value})))
    for name in CALLS:
        for k, (a, v, x, o, p) in enumerate(bad_inputs):
            rc, clean = raw(pkg, matcher, name, a, v, x, o, p, n=(len(poses), len(points), len(obs)))
            assert rc == -1 and clean, (name, k)
        for n in ((0, len(points), len(obs)), (len(poses), 0, len(obs)), (len(poses), len(points), -1)):
            rc, clean = raw(pkg, matcher, name, poses, valid, points, obs, good, n=n)
            assert rc == -1 and clean, (name, n)
        # above the limits: decided from the counts, before any buffer is read (the buffers are far too small for them)
        for n in ((4097, len(points), len(obs)), (len(poses), (1 << 24) + 1, len(obs)), (len(poses), len(points), (1 << 24) + 1)):
            rc, clean = raw(pkg, matcher, name, poses, valid, points, obs, good, n=n)
            assert rc == -4 and clean, (name, n)
        required = {"lcm_ba_error": (0,), "lcm_ba_outliers": (0, 3), "lcm_ba_optimize": (0, 1, 4), "lcm_ba_refine_map": (0, 1, 2, 4)}.get(name, (0, 1))
        for k in required:
            rc, clean = raw(pkg, matcher, name, poses, valid, points, obs, good, null=(k,))
            assert rc == -1 and clean, (name, k)
    rc, clean = raw(pkg, matcher, "lcm_ba_refine_map", poses, valid, points, obs, good)
    assert rc == 0 and not clean
    lib = pkg.load_library()
    out = [np.full(s, FILL, np.uint8) for s in (96 * len(poses), 24 * len(points), 24 * len(obs), 56)]
    rc = lib.lcm_ba_refine_map(matcher._h, poses.ctypes.data, valid.ctypes.data, len(poses), points.ctypes.data, len(points), obs.ctypes.data, len(obs),
                               C.byref(good), 17, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, None,
                               C.cast(out[3].ctypes.data, C.POINTER(pkg.capi.BaMapReport)))
    assert rc == -1 and all((b == FILL).all() for b in out)
    after = matcher.ba_optimize(poses, points, obs, good, valid=valid)
    assert all(as_bytes(a) == as_bytes(b) for a, b in zip(before[:4], after[:4]))
    # an invalid pose's contents are not looked at
    junk = poses.copy()
    junk["R"][4], junk["t"][4] = np.nan, np.inf
    got = matcher.ba_optimize(junk, points, obs, good, valid=valid)
    assert as_bytes(got[0][4]) == as_bytes(junk[4]) and as_bytes(np.delete(got[0], 4)) == as_bytes(np.delete(before[0], 4)) and as_bytes(got[1]) == as_bytes(before[1])


# ---- the chain: lcm_pose_db_detect_loops -> lcm_ba_add_loop_observations -> lcm_ba_optimize ----------------------------------------
def test_a_planted_loop_becomes_observations_and_is_adjusted(pkg):
    """Twelve cameras and 400 points; the last camera (the current frame) has no observation yet.  Its keypoints and those of
    camera 0 (the past frame) are the points' projections, their SIFT rows the same random rows: the store finds the loop, its
    verified matches become observations of the points camera 0 sees, and the adjustment then refines the current camera too."""
    c = pkg.capi
    K = (E_.FX, E_.FY, E_.CX, E_.CY)
    rng = np.random.default_rng(91)
    curr, past, n = 11, 0, 400
    cam, pt = S.pairs_per_point(12, n, 5, rng, skip=(curr,))
    m, truth = S.scene(12, n, cam, pt, 15)
    for a in (m, truth):
        a.K = K
    m.uv = B.residuals(K, truth.R[cam], truth.t[cam], truth.X[pt], np.zeros((len(cam), 2))) + rng.uniform(-0.3, 0.3, (len(cam), 2))
    rows = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    kp = [(B.residuals(K, truth.R[k][None], truth.t[k][None], truth.X, np.zeros((n, 2))) + rng.uniform(-0.3, 0.3, (n, 2))).astype(np.float32)
          for k in (past, curr)]
    order = rng.permutation(n)                                        # the past frame's rows in another order
    ep = c.default_epi_params(*K)
    with pkg.Matcher() as mt:
        assert mt.l2_db_append_kp(rows[order], kp[0][order]) == 0 and mt.l2_db_append_kp(rows, kp[1]) == 1
        cands, _, res, pres, out, pts, mask, pmask, offs, best = mt.pose_db_detect_loops(1, 1, ep)
        assert best == 0 and pres[best]["status"] == c.POSE_OK
        lo, hi = int(offs[best]), int(offs[best + 1])
        matches, keep = out[lo:hi], pmask[lo:hi]
        assert hi - lo == n and keep.sum() >= 300
        past_table = order.astype(np.int32).copy()                    # past keypoint k shows point order[k] ...
        past_table[::7] = -1                                          # ... where the map has one
        curr_table = np.full(n, -1, np.int32)
        points, obs0 = c.ba_points(m.X), c.ba_obs(m.cam, m.pt, m.uv)
        obs, added = c.ba_add_loop_observations(matches, keep, past_table, curr_table, kp[1], curr, n, obs0)
        new, want_table = B.add_loop_observations([(int(q), int(t)) for q, t in zip(matches["query_idx"], matches["train_idx"])], keep, past_table,
                                                  np.full(n, -1, np.int32), kp[1], curr)
        assert added == len(new) == len(obs) - len(obs0) and 200 < added < keep.sum() and np.array_equal(curr_table, want_table)
        assert [(int(o["cam"]), int(o["point"]), float(o["u"]), float(o["v"])) for o in obs[len(obs0):]] == new
        took = (keep != 0) & (past_table[matches["train_idx"]] >= 0)
        assert as_bytes(obs[:len(obs0)]) == as_bytes(obs0) and np.array_equal(obs["point"][len(obs0):], matches["query_idx"][took])
        poses = c.pgo_poses(m.R, m.t)
        p = bp(pkg, m)
        b0 = mt.ba_optimize(poses, points, obs0, p)
        b1 = mt.ba_optimize(poses, points, obs, p)
        assert b0[2]["status"][curr] == B.SKIPPED and as_bytes(b0[0][curr]) == as_bytes(poses[curr])
        assert b1[2]["status"][curr] in (B.CONVERGED, B.MAX_ITERS) and b1[4].mean_error[5] < 0.5 < b1[4].mean_error[0]
        new_only = mt.ba_error(b1[0], b1[1], obs[len(obs0):], p)
        assert new_only < 0.5 < mt.ba_error(poses, points, obs[len(obs0):], p)

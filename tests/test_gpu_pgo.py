"""The pose-graph correction on the device (include/lcm.h, lcm_pgo_*) through the C ABI, against tests/pgoref.py.

Tolerances: 16 x the restatement's own float64 rounding, the project's standing margin (tests/test_gpu_lo.py,
tests/test_gpu_epi.py).  The own errors are tests/pgocases.py's OWN_* constants, measured on the CPU by
tests/test_pgo_ref_host.py over these very cases: residuals and parameters 1e-15 and Jacobian entries 5e-10 per sqrt(largest
weight) (float64 against longdouble), one step's dp 2e-13 (Cholesky against lstsq on the same J), a complete run's poses 1e-9 and
its costs and last update 1e-4 relative (the same two routes)."""
import ctypes as C

import numpy as np
import pytest

import pgocases as S
import pgoref as G

pytestmark = pytest.mark.gpu
MARGIN = 16
FILL = 0xA7


def records(pkg, g):
    E = g["E"]
    return pkg.capi.pgo_poses(g["R"], g["t"]), pkg.capi.pgo_edges(E.R, E.t, E.w, np.stack([E.f, E.to], 1)), g["valid"].astype(np.uint8)


def scale(g):
    return float(np.sqrt(max(1.0, g["E"].w.max())))


_REFS = {}


def step_reference(name):
    """The case's graph and pgoref's parameters, residuals and Jacobian: computed once, shared, never written to."""
    if name not in _REFS:
        g = S.STEP_CASES[name]()
        P, _ = G.params_of(g["R"], g["t"], g["valid"])
        r, J, _ = G.linearise(P, g["R"][0], g["t"][0], g["E"])
        for a in (P, r, J):
            a.setflags(write=False)
        _REFS[name] = (g, P, r, J)
    return _REFS[name]


def run_reference(name):
    if name not in _REFS:
        mk, pp = S.RUN_CASES[name]
        g = mk()
        _REFS[name] = (g, G.run(g["R"], g["t"], g["E"], g["valid"], "a", **pp))
    return _REFS[name]


def angle_to(R, Rt):
    rv, _ = G.log(G.mm(R, G.tr(Rt)))
    return float(np.sqrt((rv * rv).sum(-1)).max())


# ---- one step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.STEP_CASES))
def test_one_step(pkg, matcher, name):
    g, Pw, rw, Jw = step_reference(name)
    n, E = len(g["R"]), g["E"]
    poses, edges, valid = records(pkg, g)
    P, r, J, dp, info = matcher.pgo_step(poses, edges, valid=valid)
    eP, er, eJ = np.abs(P - Pw).max(), np.abs(r - rw).max(), np.abs(J - Jw).max()
    print(f"{name}: params {eP:.3g}, r {er:.3g}, J {eJ:.3g} (limits {MARGIN * S.OWN_R:.3g}, {MARGIN * S.OWN_R * scale(g):.3g}, {MARGIN * S.OWN_J * scale(g):.3g})")
    assert eP <= MARGIN * S.OWN_R and er <= MARGIN * S.OWN_R * scale(g)
    assert eJ <= MARGIN * S.OWN_J * scale(g)
    # pose 0's columns do not exist; an invalid pose's parameters are zeros
    assert not J[E.f == 0][:, :, :6].any() and not J[E.to == 0][:, :, 6:].any()
    assert not P[~g["valid"]].any()
    # the closure on the device's own output: route A (the block solve where no dense matrix fits) on ITS r and J
    if name in S.LARGE:
        want, lam = G.solve_blocks(J, r, E, g["valid"], n)
    else:
        want, lam = G.solve_a(G.scatter(J, E, n), r)
    edp = np.abs(dp - want).max()
    print(f"{name}: dp {edp:.3g} (limit {MARGIN * S.OWN_DP:.3g}), max |dp| {np.abs(dp).max():.3g}")
    assert edp <= MARGIN * S.OWN_DP
    reached = np.zeros(n, bool)
    reached[E.f], reached[E.to] = True, True
    idle = ~(g["valid"] & reached)[1:]
    assert np.array_equal(dp[idle], np.zeros_like(dp[idle]))
    if name == "unreached_pose":
        assert g["valid"][6] and not reached[6]
    pl = G.plan(g["valid"], E, n)
    assert (info.iterations, info.n_border, info.n_params) == (1, len(pl["border"]), 6 * (len(pl["interior"]) + len(pl["border"])))
    assert info.status == (G.CONVERGED if np.abs(dp).max() < 1e-6 else G.MAX_ITERS)
    cost = float(r.reshape(-1) @ r.reshape(-1))
    order = 432 * len(E) * np.finfo(np.float64).eps         # two orders of a sum of 432 m non-negative products differ by at most this
    assert abs(info.lambda_ - lam) <= order * lam and abs(info.cost_first - cost) <= order * cost and info.cost_last == info.cost_first
    assert info.max_update == np.abs(dp).max()
    li = matcher.launch_info()
    assert li.pairs == len(E) and li.launches == 7 and li.kernel_ms > 0


def test_the_same_call_gives_the_same_bytes(pkg, matcher):
    """... also after a different graph has run on the handle (buffers of another shape, a longer border)."""
    first = {}
    for name in ("e65_border_at_ends", "loops8_border16", "invalid_middle"):
        g = step_reference(name)[0]
        first[name] = matcher.pgo_step(*records(pkg, g)[:2], valid=records(pkg, g)[2])
    for name in ("invalid_middle", "e65_border_at_ends", "loops8_border16", "loops8_border16"):
        g = step_reference(name)[0]
        again = matcher.pgo_step(*records(pkg, g)[:2], valid=records(pkg, g)[2])
        for a, b in zip(first[name][:4], again[:4]):
            assert a.tobytes() == b.tobytes(), name
        assert bytes(first[name][4]) == bytes(again[4]), name
    g = run_reference("ring65")[0]
    poses, edges, valid = records(pkg, g)
    a, ia = matcher.pgo_optimize(poses, edges, valid=valid)
    matcher.pgo_step(*records(pkg, step_reference("p9")[0])[:2])
    b, ib = matcher.pgo_optimize(poses, edges, valid=valid)
    assert a.tobytes() == b.tobytes() and bytes(ia) == bytes(ib)


# ---- complete runs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.RUN_CASES))
def test_complete_run(pkg, matcher, name):
    g, want = run_reference(name)
    poses, edges, valid = records(pkg, g)
    out, info = matcher.pgo_optimize(poses, edges, pkg.capi.default_pgo_params(**S.RUN_CASES[name][1]), valid=valid)
    R, t = out["R"].reshape(-1, 3, 3), out["t"]
    e = max(np.abs(R - want["R"]).max(), np.abs(t - want["t"]).max())
    rel = max(abs(getattr(info, k) - want[k]) / abs(want[k]) for k in ("cost_first", "cost_last", "max_update"))
    print(f"{name}: iterations {info.iterations}, status {info.status}, poses {e:.3g} (limit {MARGIN * S.OWN_RUN:.3g}), "
          f"costs / update relative {rel:.3g} (limit {MARGIN * S.OWN_RUN_REL:.3g})")
    assert (info.iterations, info.status) == (want["iterations"], want["status"])
    assert e <= MARGIN * S.OWN_RUN and rel <= MARGIN * S.OWN_RUN_REL
    assert out[0].tobytes() == poses[0].tobytes()
    for (past, curr), k in zip(g["loops"], range(len(g["E"]) - len(g["loops"]), len(g["E"]))):
        before = pkg.capi.pgo_rotation_drift(poses, past, curr, g["E"].R[k])
        after = pkg.capi.pgo_rotation_drift(out, past, curr, g["E"].R[k])
        assert after < before, (name, past, curr, before, after)
    li = matcher.launch_info()
    assert li.pairs == len(g["E"]) and li.launches == 2 + 5 * 20


def test_the_257_pose_run_reaches_the_iteration_limit():
    _, want = run_reference("ring257_max_iters")
    assert (want["iterations"], want["status"]) == (20, G.MAX_ITERS)


def test_invalid_poses_come_back_byte_for_byte(pkg, matcher):
    g = S.graph(12, 19, [(2, 9)], invalid=(6,))                 # updates 0.17, 7e-4, 4.6e-6, 3.3e-8: clear of min_update
    g["R"][6], g["t"][6] = np.nan, np.inf                       # an invalid pose's contents are not read
    poses, edges, valid = records(pkg, g)
    out, info = matcher.pgo_optimize(poses, edges, valid=valid)
    want = G.run(np.where(g["valid"][:, None, None], g["R"], np.eye(3)), np.where(g["valid"][:, None], g["t"], 0.0), g["E"], g["valid"], "a")
    assert out[6].tobytes() == poses[6].tobytes() and out[0].tobytes() == poses[0].tobytes()
    assert (info.iterations, info.status) == (want["iterations"], want["status"])
    keep = g["valid"]
    assert max(np.abs(out["R"].reshape(-1, 3, 3)[keep] - want["R"][keep]).max(), np.abs(out["t"][keep] - want["t"][keep]).max()) <= MARGIN * S.OWN_RUN
    aliased = poses.copy()                                       # poses_out may alias poses
    info2 = pkg.capi.PgoInfo()
    rc = matcher._lib.lcm_pgo_optimize(matcher._h, aliased.ctypes.data, valid.ctypes.data, len(aliased), edges.ctypes.data, len(edges), None,
                                       aliased.ctypes.data, C.byref(info2))
    assert rc == 0 and aliased.tobytes() == out.tobytes() and bytes(info2) == bytes(info)


def test_max_iters_1_is_the_step_seam(pkg, matcher):
    g = step_reference("p9")[0]
    poses, edges, valid = records(pkg, g)
    P, r, J, dp, si = matcher.pgo_step(poses, edges, valid=valid)
    out, info = matcher.pgo_optimize(poses, edges, pkg.capi.default_pgo_params(max_iters=1), valid=valid)
    assert bytes(info) == bytes(si) and (info.iterations, info.status) == (1, G.MAX_ITERS)
    P1 = P.copy()
    P1[1:] += dp
    assert np.abs(out["R"].reshape(-1, 3, 3)[1:] - G.exp(P1[1:, :3])).max() <= MARGIN * S.OWN_R and np.array_equal(out["t"][1:], P1[1:, 3:])


# ---- the statuses ------------------------------------------------------------------------------------------------------------
def test_a_consistent_graph_converges_in_one_iteration(pkg, matcher):
    g = S.consistent(9, 5)
    poses, edges, valid = records(pkg, g)
    P, r, J, dp, _ = matcher.pgo_step(poses, edges)
    assert not r.any() and not dp.any() and np.abs(J).max() > 0.5
    out, info = matcher.pgo_optimize(poses, edges)
    assert (info.iterations, info.status, info.max_update, info.cost_first, info.cost_last) == (1, G.CONVERGED, 0.0, 0.0, 0.0)
    assert out.tobytes() == poses.tobytes()


def test_all_weights_zero_fails_the_solve(pkg, matcher):
    g = S.graph(9, 7, [(0, 8)])
    g["E"].w[:] = 0.0
    poses, edges, valid = records(pkg, g)
    out, info = matcher.pgo_optimize(poses, edges)
    assert (info.iterations, info.status, info.lambda_, info.cost_first) == (0, G.SOLVE_FAILED, 0.0, 0.0)
    P, _ = G.params_of(g["R"], g["t"])                           # the write-back of the unmodified parameters
    assert out[0].tobytes() == poses[0].tobytes() and np.array_equal(out["t"], g["t"])
    assert np.abs(out["R"].reshape(-1, 3, 3) - G.exp(P[:, :3])).max() <= MARGIN * S.OWN_R
    P2, r, J, dp, si = matcher.pgo_step(poses, edges)
    assert si.status == G.SOLVE_FAILED and not dp.any() and not J.any()


def test_half_a_turn_ends_the_run(pkg, matcher):
    c = pkg.capi
    poses = c.pgo_poses(np.tile(np.eye(3), (3, 1, 1)), np.zeros((3, 3)))
    edges = c.pgo_edges([np.eye(3), np.diag([1.0, -1.0, -1.0])], np.zeros((2, 3)), [1.0, 1.0], [(0, 1), (1, 2)])
    out, info = matcher.pgo_optimize(poses, edges)
    assert (info.iterations, info.status) == (0, G.HALF_TURN) and out.tobytes() == poses.tobytes()
    want = G.run(np.tile(np.eye(3), (3, 1, 1)), np.zeros((3, 3)), G.Edges(edges["R"], edges["t"], edges["weight"], [(0, 1), (1, 2)]))
    assert (want["iterations"], want["status"]) == (0, G.HALF_TURN)
    turned = c.pgo_poses([np.eye(3), np.diag([-1.0, 1.0, -1.0])], np.zeros((2, 3)))      # a pose without a rotation vector
    out, info = matcher.pgo_optimize(turned, edges[:1])
    assert (info.iterations, info.status) == (0, G.HALF_TURN) and out.tobytes() == turned.tobytes()


# ---- lcm_pgo_close_loop ------------------------------------------------------------------------------------------------------
def planted(pkg):
    """A drifted ring whose loop is given as lcm_pose_* gives it: X_past = R X_curr + t."""
    g = S.graph(33, 5, [])
    past, curr = 0, 32
    R = G.mm(g["Rt"][past], G.tr(g["Rt"][curr]))
    pr = pkg.capi.PoseResult()
    pr.R[:], pr.t[:] = R.reshape(-1).tolist(), (g["tt"][past] - G.mv(R, g["tt"][curr])).tolist()
    pr.status = pkg.capi.POSE_OK
    return g, past, curr, pr


@pytest.mark.parametrize("direction", [0, 1])
def test_close_loop_is_build_graph_and_optimize(pkg, matcher, direction):
    c = pkg.capi
    g, past, curr, pr = planted(pkg)
    g["valid"][7] = False
    poses, _, valid = records(pkg, g)
    pp = c.default_pgo_params(loop_direction=direction, loop_weight=4.0)
    out, info = matcher.pgo_close_loop(poses, past, curr, pr, pp, valid=valid)
    R, t = np.array(pr.R).reshape(3, 3), np.array(pr.t)
    if direction == c.PGO_LOOP_INVERTED:
        R, t = R.T.copy(), -G.mv(R.T, t)
    edges = c.pgo_build_graph(poses, past, curr, R, t, pp, valid=valid)
    assert len(edges) == 31 and edges[-1]["weight"] == 4.0 and (edges[-1]["from"], edges[-1]["to"]) == (past, curr)
    want, winfo = matcher.pgo_optimize(poses, edges, pp, valid=valid)
    assert out.tobytes() == want.tobytes() and bytes(info) == bytes(winfo)


def test_the_inverted_direction_is_the_consistent_one(pkg, matcher):
    """On a planted scene INVERTED lowers the distance to the true poses; AS_WRITTEN, the reference's lines, does not."""
    c = pkg.capi
    g, past, curr, pr = planted(pkg)
    poses = records(pkg, g)[0]
    before = angle_to(g["R"], g["Rt"])
    got = {}
    for d in (c.PGO_LOOP_AS_WRITTEN, c.PGO_LOOP_INVERTED):
        out, info = matcher.pgo_close_loop(poses, past, curr, pr, c.default_pgo_params(loop_direction=d))
        got[d] = angle_to(out["R"].reshape(-1, 3, 3), g["Rt"])
    print(f"largest rotation error to the true poses: {before:.4g} rad before, {got[0]:.4g} as written, {got[1]:.4g} inverted")
    assert got[c.PGO_LOOP_INVERTED] < before <= got[c.PGO_LOOP_AS_WRITTEN]
    default, _ = matcher.pgo_close_loop(poses, past, curr, pr)
    assert angle_to(default["R"].reshape(-1, 3, 3), g["Rt"]) == got[c.PGO_LOOP_AS_WRITTEN]


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def raw_calls(pkg, m, poses, valid, n, edges, n_edges, pp, null=()):
    """lcm_pgo_optimize and lcm_pgo_step on pre-filled outputs: ([rc, rc], every output still holds its fill)."""
    bufs = {k: np.full(sz, FILL, np.uint8) for k, sz in (("out", 96 * 80), ("info", 48), ("params", 48 * 80), ("res", 48 * 80),
                                                           ("jac", 576 * 80), ("dp", 48 * 80))}
    p = {k: (None if k in null else b.ctypes.data) for k, b in bufs.items()}
    pa = None if "poses" in null else poses.ctypes.data
    ea = None if "edges" in null else edges.ctypes.data
    va = None if valid is None else valid.ctypes.data
    ppp = None if pp is None else C.byref(pp)
    lib = m._lib
    rcs = [lib.lcm_pgo_optimize(m._h, pa, va, n, ea, n_edges, ppp, p["out"], C.cast(p["info"], C.POINTER(pkg.capi.PgoInfo))),
           lib.lcm_pgo_step(m._h, pa, va, n, ea, n_edges, ppp, p["params"], p["res"], p["jac"], p["dp"],
                            C.cast(p["info"], C.POINTER(pkg.capi.PgoInfo)))]
    return rcs, all((b == FILL).all() for b in bufs.values())


def test_refusals_write_nothing_and_leave_the_handle_usable(pkg, matcher):
    c = pkg.capi
    g = S.graph(9, 7, [(0, 8)])
    poses, edges, valid = records(pkg, g)
    n, m = len(poses), len(edges)

    def with_edge(**kw):
        e = edges.copy()
        for k, v in kw.items():
            e[4][k] = v
        return e

    def with_pose(**kw):
        p = poses.copy()
        for k, v in kw.items():
            p[3][k] = v
        return p

    skew = np.eye(3).reshape(-1).copy()
    skew[1] = 1e-5
    nan_R, inf_t, mirror = np.full(9, np.nan), np.array([0.0, np.inf, 0.0]), np.diag([1.0, 1.0, -1.0]).reshape(-1)
    invalid3, invalid0 = valid.copy(), valid.copy()
    invalid3[3], invalid0[0] = 0, 0
    bad = [("n_poses < 2", dict(n=1)), ("n_edges < 1", dict(n_edges=0)), ("negative n_poses", dict(n=-4)),
           ("pose 0 invalid", dict(valid=invalid0)), ("an invalid endpoint", dict(valid=invalid3)),
           ("from == to", dict(edges=with_edge(to=4))), ("index below 0", dict(edges=with_edge(**{"from": -1}))),
           ("index past the end", dict(edges=with_edge(to=n))),
           ("negative weight", dict(edges=with_edge(weight=-1.0))), ("NaN weight", dict(edges=with_edge(weight=np.nan))),
           ("infinite weight", dict(edges=with_edge(weight=np.inf))),
           ("NaN in an edge's R", dict(edges=with_edge(R=nan_R))), ("Inf in an edge's t", dict(edges=with_edge(t=inf_t))),
           ("NaN in a pose's R", dict(poses=with_pose(R=nan_R))), ("Inf in a pose's t", dict(poses=with_pose(t=inf_t))),
           ("a pose's R not orthonormal", dict(poses=with_pose(R=skew))), ("an edge's R not orthonormal", dict(edges=with_edge(R=skew))),
           ("a pose's R a reflection", dict(poses=with_pose(R=mirror))), ("an edge's R a reflection", dict(edges=with_edge(R=mirror)))]
    bad += [(f"pp.{k} = {v}", dict(pp=c.default_pgo_params(**{k: v}))) for k, v in
            (("eps", 0.0), ("eps", -1e-6), ("eps", np.nan), ("eps", np.inf), ("damping", -1.0), ("damping", np.nan), ("min_update", -1.0),
             ("min_update", np.inf), ("loop_weight", -1.0), ("loop_weight", np.nan), ("max_iters", 0), ("max_iters", 101),
             ("loop_direction", 2), ("loop_direction", -1))]
    for what, kw in bad:
        rcs, untouched = raw_calls(pkg, matcher, kw.get("poses", poses), kw.get("valid", valid), kw.get("n", n), kw.get("edges", edges),
                                   kw.get("n_edges", m), kw.get("pp"))
        assert rcs == [-1, -1] and untouched, (what, rcs)
        assert matcher._lib.lcm_last_error() != b""
    for null in ("poses", "edges", "info"):
        rcs, untouched = raw_calls(pkg, matcher, poses, valid, n, edges, m, None, null=(null,))
        assert rcs == [-1, -1] and untouched, null
    for null, which in (("out", 0), ("params", 1), ("res", 1), ("jac", 1), ("dp", 1)):
        rcs, untouched = raw_calls(pkg, matcher, poses, valid, n, edges, m, None, null=(null,))
        assert rcs[which] == -1 and rcs[1 - which] == 0, null
    # lcm_pgo_close_loop: a pose that is not LCM_POSE_OK, bad ends, NULLs
    pr = c.PoseResult()
    pr.R[:] = np.eye(3).reshape(-1).tolist()
    out, info = np.full(96 * 16, FILL, np.uint8), np.full(48, FILL, np.uint8)
    ip = C.cast(info.ctypes.data, C.POINTER(c.PgoInfo))
    lib, h = matcher._lib, matcher._h
    pr.status = c.POSE_NO_MODEL
    assert lib.lcm_pgo_close_loop(h, poses.ctypes.data, None, n, 0, 8, C.byref(pr), None, out.ctypes.data, ip) == -1
    pr.status = c.POSE_OK
    for past, curr, vv in ((0, 9, None), (-1, 8, None), (4, 4, None), (3, 8, invalid3)):
        assert lib.lcm_pgo_close_loop(h, poses.ctypes.data, None if vv is None else vv.ctypes.data, n, past, curr, C.byref(pr), None,
                                      out.ctypes.data, ip) == -1, (past, curr)
    assert lib.lcm_pgo_close_loop(h, poses.ctypes.data, None, n, 0, 8, None, None, out.ctypes.data, ip) == -1
    assert lib.lcm_pgo_close_loop(h, poses.ctypes.data, None, n, 0, 8, C.byref(pr), C.byref(c.default_pgo_params(max_iters=0)), out.ctypes.data, ip) == -1
    assert (out == FILL).all() and (info == FILL).all()
    # the handle is usable afterwards
    P, r, J, dp, si = matcher.pgo_step(poses, edges, valid=valid)
    assert si.iterations == 1 and np.abs(J).max() > 0.5


def test_limits(pkg, matcher):
    c = pkg.capi
    n = c.PGO_MAX_POSES + 1
    poses = c.pgo_poses(np.tile(np.eye(3), (n, 1, 1)), np.arange(3 * n).reshape(n, 3) % 7)
    ends = [(i - 1, i) for i in range(1, n)]
    edges = c.pgo_edges(np.tile(np.eye(3), (n - 1, 1, 1)), poses["t"][1:] - poses["t"][:-1], np.ones(n - 1), ends)
    rcs, untouched = raw_calls(pkg, matcher, poses, None, n, edges, n - 1, None)
    assert rcs == [-4, -4] and untouched                                        # LCM_ERR_CAPACITY
    rcs, _ = raw_calls(pkg, matcher, poses, None, 64, edges, 63, None)
    assert rcs == [0, 0]
    loops = [(k, k + 20) for k in range(c.PGO_MAX_LOOPS + 1)]
    more = c.pgo_edges(np.tile(np.eye(3), (9, 1, 1)), [poses["t"][b] - poses["t"][a] for a, b in loops], np.ones(9), loops)
    rcs, untouched = raw_calls(pkg, matcher, poses, None, 64, np.concatenate([edges[:63], more]), 72, None)
    assert rcs == [-4, -4] and untouched
    rcs, _ = raw_calls(pkg, matcher, poses, None, 64, np.concatenate([edges[:63], more[:8]]), 71, None)
    assert rcs == [0, 0]
    pr = c.PoseResult()
    pr.R[:] = np.eye(3).reshape(-1).tolist()
    info = c.PgoInfo()
    out = np.zeros(n, c.PGO_POSE_DTYPE)
    assert matcher._lib.lcm_pgo_close_loop(matcher._h, poses.ctypes.data, None, n, 0, n - 1, C.byref(pr), None, out.ctypes.data, C.byref(info)) == -4

"""The pose-graph correction's numpy restatement (tests/pgoref.py) on the CPU: what its own float64 rounding is worth, that the
iteration counts of the complete runs cannot turn on rounding, that the correction lowers the drift, and that the block-sparse
Jacobian is the reference's dense one exactly.  The own errors measured here are the constants OWN_* of tests/pgocases.py, from
which tests/test_gpu_pgo.py takes the device's tolerances (16 x, the project's standing margin)."""
import numpy as np
import pytest

import pgocases as S
import pgoref as G

LD = np.longdouble


def scale(g):
    """Residuals and Jacobian entries are proportional to sqrt(weight): their own error is measured per unit of it."""
    return float(np.sqrt(max(1.0, g["E"].w.max())))


@pytest.fixture(scope="module")
def graphs():
    out = {name: mk() for name, mk in S.STEP_CASES.items()}
    out.update({name: mk() for name, (mk, _) in S.RUN_CASES.items()})
    return out


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name, (mk, pp) in S.RUN_CASES.items():
        g = mk()
        out[name] = (g, G.run(g["R"], g["t"], g["E"], g["valid"], "a", **pp), G.run(g["R"], g["t"], g["E"], g["valid"], "b", **pp))
    return out


def test_own_error_of_the_linearisation(graphs):
    worst_r = worst_j = 0.0
    for name, g in graphs.items():
        P, ok = G.params_of(g["R"], g["t"], g["valid"])
        r, J, ok2 = G.linearise(P, g["R"][0], g["t"][0], g["E"])
        rl, Jl, _ = G.linearise(P, g["R"][0], g["t"][0], g["E"], dt=LD)
        assert ok and ok2, name
        er, ej = float(np.abs(r - rl).max()) / scale(g), float(np.abs(J - Jl).max()) / scale(g)
        print(f"{name:24s} r {er:.3g} J {ej:.3g} (per sqrt(weight) {scale(g):.4g})")
        worst_r, worst_j = max(worst_r, er), max(worst_j, ej)
    print(f"worst: r {worst_r:.3g} (OWN_R {S.OWN_R:.3g}), J {worst_j:.3g} (OWN_J {S.OWN_J:.3g})")
    assert worst_r <= S.OWN_R and worst_j <= S.OWN_J


def test_own_error_of_one_step(graphs):
    worst_ab = worst_blocks = 0.0
    for name, g in graphs.items():
        n = len(g["R"])
        P, _ = G.params_of(g["R"], g["t"], g["valid"])
        r, J, _ = G.linearise(P, g["R"][0], g["t"][0], g["E"])
        blocks, lam_b = G.solve_blocks(J, r, g["E"], g["valid"], n)
        if name in S.LARGE:                                        # no dense matrix: float64 against longdouble in the block solve
            exact, _ = G.solve_blocks(J, r, g["E"], g["valid"], n, dt=LD)
            eb = float(np.abs(blocks - exact).max())
            print(f"{name:24s} blocks float64 - longdouble {eb:.3g}")
        else:
            Jd = G.scatter(J, g["E"], n)
            a, lam_a = G.solve_a(Jd, r)
            b, _ = G.solve_b(Jd, r)
            eab, eb = float(np.abs(a - b).max()), float(np.abs(blocks - a).max())
            assert abs(lam_a - lam_b) <= 1e-14 * lam_a
            print(f"{name:24s} A - B {eab:.3g}, blocks - A {eb:.3g}")
            worst_ab = max(worst_ab, eab)
        worst_blocks = max(worst_blocks, eb)
    print(f"worst: A - B {worst_ab:.3g} (OWN_DP {S.OWN_DP:.3g}), the block solve {worst_blocks:.3g}")
    assert worst_ab <= S.OWN_DP
    assert worst_blocks <= S.OWN_DP            # the block solve stands in for route A where no dense matrix fits


def test_own_error_of_a_complete_run(runs):
    worst = worst_rel = 0.0
    for name, (g, a, b) in runs.items():
        e = max(float(np.abs(a["R"] - b["R"]).max()), float(np.abs(a["t"] - b["t"]).max()))
        rel = max(abs(a[k] - b[k]) / abs(a[k]) for k in ("cost_first", "cost_last", "max_update"))
        print(f"{name:20s} iterations {a['iterations']} status {a['status']}: poses A - B {e:.3g}, cost / update relative {rel:.3g}")
        assert (a["iterations"], a["status"]) == (b["iterations"], b["status"]), name
        worst, worst_rel = max(worst, e), max(worst_rel, rel)
    print(f"worst: poses {worst:.3g} (OWN_RUN {S.OWN_RUN:.3g}), relative {worst_rel:.3g} (OWN_RUN_REL {S.OWN_RUN_REL:.3g})")
    assert worst <= S.OWN_RUN and worst_rel <= S.OWN_RUN_REL
    assert [runs[k][1]["iterations"] for k in ("ring3", "ring9", "ring65", "eight65_3loops")] == [3, 3, 6, 5]
    assert (runs["ring257_max_iters"][1]["iterations"], runs["ring257_max_iters"][1]["status"]) == (20, G.MAX_ITERS)


def test_stopping_margin(runs):
    """No max_update of any run, under either route, lies within a factor 2 of min_update: the iteration count cannot turn on
    rounding."""
    lo, hi = G.DEFAULTS["min_update"] / 2, G.DEFAULTS["min_update"] * 2
    for name, (g, a, b) in runs.items():
        for res in (a, b):
            print(name, ["%.3g" % u for u in res["updates"]])
            assert all(u < lo or u > hi for u in res["updates"]), (name, res["updates"])


def test_the_correction_lowers_the_drift(runs):
    for name, (g, a, b) in runs.items():
        for (past, curr), e in zip(g["loops"], range(len(g["E"]) - len(g["loops"]), len(g["E"]))):
            before = G.rotation_drift(g["R"], past, curr, g["E"].R[e])
            after = G.rotation_drift(a["R"], past, curr, g["E"].R[e])
            print(f"{name:20s} loop {past} -> {curr}: drift {before:.4g} -> {after:.4g} rad")
            assert after < before, name
        assert a["cost_last"] < a["cost_first"]


def test_a_consistent_graph_is_left_alone():
    g = S.consistent(9, 5)
    P, ok = G.params_of(g["R"], g["t"])
    r, J, ok2 = G.linearise(P, g["R"][0], g["t"][0], g["E"])
    assert ok and ok2 and not r.any() and np.abs(J).max() > 0.5
    for route in ("a", "blocks"):
        res = G.run(g["R"], g["t"], g["E"], route=route)
        assert (res["iterations"], res["status"], res["max_update"], res["cost_first"]) == (1, G.CONVERGED, 0.0, 0.0), route
        assert np.array_equal(res["R"], g["R"]) and np.array_equal(res["t"], g["t"])


@pytest.mark.parametrize("name", ["one_edge", "p3", "p9", "e17_shared_endpoint", "invalid_middle", "unreached_pose", "duplicates",
                                  "weights_0_1e6"])
def test_block_sparse_jacobian_is_the_dense_one_exactly(name):
    """src/main.cpp:345-407 transcribed (every column re-evaluates every edge) gives the twelve columns per edge bit for bit:
    outside an edge's two poses r_plus - r_minus is 0.0."""
    g = S.STEP_CASES[name]()
    n = len(g["R"])
    P, _ = G.params_of(g["R"], g["t"], g["valid"])
    r, J, _ = G.linearise(P, g["R"][0], g["t"][0], g["E"])
    rd, Jd = G.dense_reference(P, g["R"][0], g["t"][0], g["E"])
    assert np.array_equal(rd, r.reshape(-1))
    assert np.array_equal(Jd, G.scatter(J, g["E"], n))


def test_log_and_exp():
    rng = np.random.default_rng(3)
    rv = rng.standard_normal((200, 3))
    rv *= (rng.uniform(0.0, 3.1, 200) / np.linalg.norm(rv, axis=1))[:, None]
    back, ok = G.log(G.exp(rv))
    assert ok.all() and np.abs(back - rv).max() < 1e-12
    assert np.array_equal(G.exp(np.zeros(3)), np.eye(3)) and np.array_equal(G.exp(np.full(3, 1e-17)), np.eye(3))
    small, ok = G.log(G.exp(np.array([3e-6, -2e-6, 1e-6])))               # below s = 1e-5: v itself, not OpenCV's zero vector
    assert ok and np.abs(small - [3e-6, -2e-6, 1e-6]).max() < 1e-16 and small.any()
    _, ok = G.log(np.diag([1.0, -1.0, -1.0]))
    assert not ok
    _, ok = G.log(G.exp(np.array([0.0, np.pi - 1e-3, 0.0])))
    assert ok

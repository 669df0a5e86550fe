"""Seeded trajectories for the pose-graph correction's tests: a camera on a ring or on a figure of eight, its odometry drifting by a
small rotation and translation per edge, the poses handed to the optimiser chained from that odometry (so that the sequential
edges, built from them as src/main.cpp:1444-1460 builds them, start at a zero residual), and loop edges taken from the TRUE poses.
STEP_CASES are the one-iteration shapes of tests/test_gpu_pgo.py, RUN_CASES its complete runs."""
import numpy as np

import pgoref as G


# float64's own rounding in the restatement, measured by tests/test_pgo_ref_host.py (which prints every figure and asserts that
# none exceeds these) as the worst over STEP_CASES and RUN_CASES; the device's tolerances are 16 x these (tests/test_gpu_pgo.py).
OWN_R = 1e-15    # residuals (and the parameters, the same log), float64 against longdouble, per sqrt(largest weight): measured 9.5e-16
OWN_J = 5e-10    # Jacobian entries, likewise: measured 4.5e-10 (the central difference divides the residual's rounding by 2e-6)
OWN_DP = 2e-13   # one step's dp on the same J, route A against route B: measured 1.06e-13 (257 poses)
OWN_RUN = 1e-9   # a complete run's poses, route A against route B: measured 8.5e-10 (257 poses, 20 iterations)
OWN_RUN_REL = 1e-4   # ... and its cost_first, cost_last and max_update, relative: measured 8.9e-5 (a last update of 2e-7)


def true_poses(n, kind, rng):
    """World-to-camera poses (R [n, 3, 3], t [n, 3]) of a camera at c_i looking along a slowly turning heading."""
    s = np.arange(n) / max(n, 2)
    phi = 2 * np.pi * s
    if kind == "ring":
        c = np.stack([5 * np.cos(phi), 0.3 * np.sin(3 * phi), 5 * np.sin(phi)], 1)
    else:                                                         # a figure of eight
        c = np.stack([5 * np.sin(phi), 0.3 * np.cos(2 * phi), 3 * np.sin(2 * phi)], 1)
    rv = np.stack([0.2 * np.sin(2 * phi), 2.4 * s, 0.15 * np.cos(phi)], 1) + 0.02 * rng.standard_normal((n, 3))
    R = G.exp(rv)
    return R, -G.mv(R, c)


def chain(Rt, tt, drift, rng):
    """The poses dead reckoning gives: every true relative motion turned by `drift` rad about a random axis and shifted."""
    n = len(Rt)
    R, t = Rt.copy(), tt.copy()
    for i in range(1, n):
        R_rel = G.mm(Rt[i], G.tr(Rt[i - 1]))
        t_rel = tt[i] - G.mv(R_rel, tt[i - 1])
        axis = rng.standard_normal(3)
        R_rel = G.mm(G.exp(drift * axis / np.linalg.norm(axis)), R_rel)
        t_rel = t_rel + 2 * drift * rng.standard_normal(3)
        R[i], t[i] = G.mm(R_rel, R[i - 1]), G.mv(R_rel, t[i - 1]) + t_rel
    return R, t


def true_edge(Rt, tt, a, b):
    R_rel = G.mm(Rt[b], G.tr(Rt[a]))
    return R_rel, tt[b] - G.mv(R_rel, tt[a])


def graph(n, seed, loops, kind="ring", drift=0.01, invalid=(), loop_weight=10.0, extra=(), weights=None):
    """dict(R, t: the drifted poses; Rt, tt: the true ones; valid; E: the sequential edges of the valid poses, then one loop edge
    (past, curr) per entry of `loops` from the true poses, then copies of the edges whose indices `extra` lists).  weights:
    {edge index: weight} overrides."""
    rng = np.random.default_rng(seed)
    Rt, tt = true_poses(n, kind, rng)
    R, t = chain(Rt, tt, drift, rng)
    valid = np.ones(n, bool)
    valid[list(invalid)] = False
    Rs, ts, ws, ends = [], [], [], []
    for i in range(1, n):
        if valid[i - 1] and valid[i]:
            R_rel = G.mm(R[i], G.tr(R[i - 1]))
            Rs.append(R_rel), ts.append(t[i] - G.mv(R_rel, t[i - 1])), ws.append(1.0), ends.append((i - 1, i))
    for a, b in loops:
        R_rel, t_rel = true_edge(Rt, tt, a, b)
        Rs.append(R_rel), ts.append(t_rel), ws.append(loop_weight), ends.append((a, b))
    for e in extra:
        Rs.append(Rs[e]), ts.append(ts[e]), ws.append(ws[e]), ends.append(ends[e])
    for e, w in (weights or {}).items():
        ws[e] = w
    return dict(R=R, t=t, Rt=Rt, tt=tt, valid=valid, E=G.Edges(Rs, ts, ws, ends), loops=list(loops))


def single_edge(seed):
    """Two poses and one edge from pose 0, measured on the true poses: one block, no coupling."""
    g = graph(2, seed, [])
    R_rel, t_rel = true_edge(g["Rt"], g["tt"], 0, 1)
    g["E"] = G.Edges([R_rel], [t_rel], [1.0], [(0, 1)])
    return g


def consistent(n, seed):
    """Exact odometry and a loop edge equal to the sequential composition, in numbers every product and sum of which is exact
    (identity rotations, whose exp(log) is the identity again, and integer translations): r = 0, dp = 0, one iteration."""
    rng = np.random.default_rng(seed)
    R = np.tile(np.eye(3), (n, 1, 1))
    t = np.cumsum(rng.integers(-3, 4, (n, 3)), 0).astype(np.float64)
    ends = [(i - 1, i) for i in range(1, n)] + [(1, n - 1)]
    E = G.Edges([np.eye(3)] * n, [t[b] - t[a] for a, b in ends], [1.0] * (n - 1) + [10.0], ends)
    return dict(R=R, t=t, Rt=R, tt=t, valid=np.ones(n, bool), E=E, loops=[(1, n - 1)])


# name -> graph: the smallest shapes at which each stage can go wrong (edges = poses - 1 + loops where nothing is invalid)
STEP_CASES = {
    "one_edge": lambda: single_edge(3),
    "p3": lambda: graph(3, 7, [(0, 2)]),
    "p9": lambda: graph(9, 7, [(0, 8)]),
    "e16_loop_to_pose0": lambda: graph(16, 11, [(0, 15)]),
    "e17_shared_endpoint": lambda: graph(16, 12, [(2, 15), (2, 9)]),
    "e64_adjacent_border": lambda: graph(63, 13, [(10, 40), (11, 62)]),
    "e65_border_at_ends": lambda: graph(65, 14, [(1, 64)]),
    "e257": lambda: graph(257, 15, [(3, 250)]),
    "loops8_border16": lambda: graph(40, 16, [(1 + 2 * k, 38 - 2 * k) for k in range(8)], kind="eight"),
    "invalid_middle": lambda: graph(12, 17, [(2, 9)], invalid=(6,)),
    "unreached_pose": lambda: graph(12, 18, [(2, 9)], invalid=(5, 7)),
    "duplicates": lambda: graph(9, 19, [(0, 8)], extra=(8, 3, 8)),
    "weights_0_1e6": lambda: graph(9, 20, [(0, 8)], loop_weight=1e6, weights={4: 0.0}),
    "p4096": lambda: graph(4096, 21, [(1, 4095)], drift=0.0005),
}
LARGE = {"p4096"}                      # too large for a dense matrix: checked against pgoref.solve_blocks alone

# name -> (graph, parameters): complete runs; the seeds keep every max_update outside [min_update / 2, 2 min_update]
RUN_CASES = {
    "ring3": (lambda: graph(3, 7, [(0, 2)]), {}),
    "ring9": (lambda: graph(9, 2, [(0, 8)]), {}),
    "ring65": (lambda: graph(65, 25, [(0, 64)]), {}),
    "eight65_3loops": (lambda: graph(65, 12, [(2, 34), (10, 60), (0, 64)], kind="eight"), {}),
    "ring257_max_iters": (lambda: graph(257, 7, [(0, 256)]), {}),
}

"""Times the pose-graph correction on the device (lcm_pgo_optimize, lcm_pgo_close_loop; lcm_pgo.hip), in one process and one run.

Graphs: a camera on a ring of --sizes poses (numpy default_rng(43)), its odometry drifting by 0.002 rad and 0.004 units per edge,
the poses chained from that odometry, the sequential edges built from them by lcm_pgo_build_graph and ONE loop edge pose 0 ->
the last pose from the true poses.  min_update = 0, so all 20 iterations run.

  optimize   lcm_pgo_optimize per size: kernel_ms (all 2 + 5 x 20 launches between the call's two events) and wall time; one
             iteration through lcm_pgo_step beside it.
  chain      at 64 poses: tools/lo_time.py's frames in the SIFT store, lcm_lo_db_detect_loops for the last frame, then
             lcm_pgo_close_loop on the best candidate's relative pose: wall time of the search alone and of both.

Warm-up calls, then --calls timed calls; median (min - max).  kernel_ms is per call: tools/pgo_trace.py splits it per kernel from
a kernel trace of this tool and appends that to the profile.

    python tools/pgo_time.py           # writes profiles/pgo_time.txt and prints it
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as entry  # noqa: E402
from epi_time import CX, CY, FX, FY, mmm, scene  # noqa: E402


def rodrigues(np, rv):
    th = np.linalg.norm(rv, axis=-1)[..., None, None]
    k = rv / np.maximum(th[..., 0], 1e-300)
    K = np.zeros(rv.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 2], k[..., 1], k[..., 2], -k[..., 0], -k[..., 1], k[..., 0]
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * k[..., :, None] * k[..., None, :] + np.sin(th) * K


def ring(np, rng, n, drift=0.002):
    """(drifted poses R, t, true poses R, t)"""
    s = np.arange(n) / n
    phi = 2 * np.pi * s
    c = np.stack([5 * np.cos(phi), 0.3 * np.sin(3 * phi), 5 * np.sin(phi)], 1)
    Rt = rodrigues(np, np.stack([0.2 * np.sin(2 * phi), 2.4 * s, 0.15 * np.cos(phi)], 1) + 0.02 * rng.standard_normal((n, 3)))
    tt = -np.einsum("nij,nj->ni", Rt, c)
    R, t = Rt.copy(), tt.copy()
    for i in range(1, n):
        R_rel = Rt[i] @ Rt[i - 1].T
        t_rel = tt[i] - R_rel @ tt[i - 1]
        axis = rng.standard_normal(3)
        R_rel = rodrigues(np, drift * axis / np.linalg.norm(axis)) @ R_rel
        R[i], t[i] = R_rel @ R[i - 1], R_rel @ t[i - 1] + t_rel + 2 * drift * rng.standard_normal(3)
    return R, t, Rt, tt


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--shared", type=int, default=300)
    ap.add_argument("--gap", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgo_time.txt"))
    args = ap.parse_args()

    import numpy as np
    pkg = entry.load_package()
    c = pkg.capi
    rng = np.random.default_rng(43)
    lines = [f"pgo_time: ring trajectories, one loop edge pose 0 -> the last pose, 20 iterations forced (min_update = 0), {args.calls} timed calls "
             f"after {args.warmup} warm-up calls"]
    forced = c.default_pgo_params(min_update=0.0)
    with pkg.Matcher() as m:
        for n in args.sizes:
            R, t, Rt, tt = ring(np, rng, n)
            poses = c.pgo_poses(R, t)
            R_loop = Rt[n - 1] @ Rt[0].T
            edges = c.pgo_build_graph(poses, 0, n - 1, R_loop, tt[n - 1] - R_loop @ tt[0])
            before = c.pgo_rotation_drift(poses, 0, n - 1, R_loop)
            kernel, wall, step = [], [], []
            for k in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                out, info = m.pgo_optimize(poses, edges, forced)
                w = (time.perf_counter() - t0) * 1e3
                i = m.launch_info()
                m.pgo_step(poses, edges)
                s_ms = m.launch_info().kernel_ms
                if k >= args.warmup:
                    kernel.append(i.kernel_ms), wall.append(w), step.append(s_ms)
            assert (info.iterations, info.status, i.launches) == (20, c.PGO_MAX_ITERS, 102)
            after = c.pgo_rotation_drift(out, 0, n - 1, R_loop)
            lines.append(f"optimize {n:5d} poses, {len(edges):5d} edges: kernel_ms {mmm(kernel)} | wall_ms {mmm(wall)} | one iteration (lcm_pgo_step) "
                         f"kernel_ms {mmm(step)} | cost {info.cost_first:.4g} -> {info.cost_last:.4g}, drift {before:.4g} -> {after:.4g} rad")

        # the chain: tools/lo_time.py's store and search, then the correction of a 64-pose trajectory on its best loop
        n = 64
        rng = np.random.default_rng(41)
        pool = rng.integers(0, 256, (args.shared, 128), dtype=np.uint8)
        corr = scene(np, rng, args.shared, args.shared // 5)
        curr = n - 1
        for f in range(n):
            rows = rng.integers(0, 256, (args.rows, 128), dtype=np.uint8)
            at = rng.permutation(args.rows)[: args.shared]
            rows[at] = np.clip(pool.astype(np.int16) + rng.integers(-3, 4, pool.shape), 0, 255).astype(np.uint8)
            kp = np.stack([rng.uniform(0, 640, args.rows), rng.uniform(0, 480, args.rows)], axis=1).astype(np.float32)
            kp[at] = corr[:, :2] if f == curr else corr[:, 2:]
            m.l2_db_append_kp(rows, kp)
        ep = c.default_epi_params(FX, FY, CX, CY)
        rule = dict(ratio=0.7, min_rows=1, min_matches=200)
        R, t, _, _ = ring(np, np.random.default_rng(43), n)
        poses = c.pgo_poses(R, t)

        def search(cap=None):
            return m.lo_db_detect_loops(curr, args.gap, ep, cand_cap=n, cap=cap, **rule)

        def chain(cap=None):
            r = search(cap)
            cands, pres, best = r[0], r[4], r[-1]
            past = int(cands[best]["matched_frame_id"])
            return m.pgo_close_loop(poses, past, curr, pres[best], forced), past, len(r[5])

        (out, info), past, total = chain()
        w_search, w_chain = [], []
        for k in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            search(total)
            t1 = time.perf_counter()
            chain(total)
            t2 = time.perf_counter()
            if k >= args.warmup:
                w_search.append((t1 - t0) * 1e3), w_chain.append((t2 - t1) * 1e3)
        lines.append(f"chain at {n} poses: lcm_lo_db_detect_loops (slot {curr} against {curr - args.gap + 1} slots, {total} survivors, best loop slot "
                     f"{past}) wall_ms {mmm(w_search)} | the same followed by lcm_pgo_close_loop ({info.iterations} iterations) wall_ms {mmm(w_chain)}")
        lines.append(f"the correction adds {statistics.median(w_chain) - statistics.median(w_search):.3f} ms of wall time (median to median) to a "
                     f"search of {statistics.median(w_search):.3f} ms")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()

"""Times the loop verification on the device (lcm_epi_db_detect_loops; lcm_epi.hip) against the candidate search with
lists and point pairs that it extends (lcm_l2_db_detect_loops_points), in one process and one run.

Frames: tools/l2_points_time.py's (--frames stored frames x --rows rows of uniform random bytes, --shared rows of every frame
copies of one pool with noise of -3..3 per byte, numpy default_rng(41)), with keypoints from a two-view scene: pool row j is a
3-D point seen by the last frame's camera (the query side) and by a second camera that every other frame stands for
(K = 700, 700, 320, 240); a fifth of the pool rows get uniformly random train-side coordinates instead.  The other rows'
keypoints are uniformly random.

  online   the last stored frame against the slots [0, last - gap] (query == NULL form, min_matches = 200):
           (a) lcm_l2_db_detect_loops_points;
           (b) lcm_epi_db_detect_loops (the same, then k_epi_solve, k_epi_score, k_epi_mask on the device's point records).
  kernels  lcm_epi_verify_pairs on (a)'s point pairs at iters 256, 1024 and 4096: kernel_ms is the three kernels' own time.

The outputs of the two routes are compared byte for byte first, then: warm-up calls of both routes and --calls timed calls
ALTERNATING between them; kernel_ms, aux_kernel_ms and wall time as median (min - max).

    python tools/epi_time.py            # writes profiles/epi_time.txt and prints it
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402

FX = FY = 700.0
CX, CY = 320.0, 240.0


def mmm(v):
    return f"{statistics.median(v):8.3f} ({min(v):8.3f} - {max(v):8.3f})"


def scene(np, rng, n, n_false):
    """float32[n, 4] (qx, qy, tx, ty): n - n_false true correspondences of two cameras, n_false with random train sides."""
    w = np.array([0.04, -0.11, 0.03])
    th = np.linalg.norm(w)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    rot = np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 10, n)], axis=1)
    X2 = X @ rot.T + np.array([0.6, -0.15, 0.2])
    pts = np.stack([FX * X[:, 0] / X[:, 2] + CX, FY * X[:, 1] / X[:, 2] + CY, FX * X2[:, 0] / X2[:, 2] + CX, FY * X2[:, 1] / X2[:, 2] + CY], axis=1)
    false = rng.permutation(n)[:n_false]
    pts[false, 2] = rng.uniform(0, 640, n_false)
    pts[false, 3] = rng.uniform(0, 480, n_false)
    return pts.astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ratio", type=float, default=0.7)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--shared", type=int, default=300)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--gap", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epi_time.txt"))
    args = ap.parse_args()

    import numpy as np
    pkg = entry.load_package()
    rng = np.random.default_rng(41)
    pool = rng.integers(0, 256, (args.shared, 128), dtype=np.uint8)
    corr = scene(np, rng, args.shared, args.shared // 5)
    curr = args.frames - 1
    frames, kps = [], []
    for f in range(args.frames):
        rows = rng.integers(0, 256, (args.rows, 128), dtype=np.uint8)
        at = rng.permutation(args.rows)[: args.shared]
        rows[at] = np.clip(pool.astype(np.int16) + rng.integers(-3, 4, pool.shape), 0, 255).astype(np.uint8)
        kp = np.stack([rng.uniform(0, 640, args.rows), rng.uniform(0, 480, args.rows)], axis=1).astype(np.float32)
        kp[at] = corr[:, :2] if f == curr else corr[:, 2:]
        frames.append(rows)
        kps.append(kp)
    lines = [f"epi_time: {args.frames} stored frames x {args.rows} rows, {args.shared} shared rows per frame ({args.shared - args.shared // 5} true "
             f"correspondences of a two-view scene, {args.shared // 5} false), ratio {args.ratio}, {args.calls} timed calls per route after "
             f"{args.warmup} warm-up calls, the two routes alternating"]
    rule = dict(ratio=args.ratio, min_rows=1, min_matches=200)

    with pkg.Matcher() as m:
        for k in ("LCM_TUNE_L2_CHUNK", "LCM_TUNE_L2_COUNT_CHUNK"):
            os.environ.pop(k, None)
        for f, kp in zip(frames, kps):
            m.l2_db_append_kp(f, kp)
        ep = pkg.capi.default_epi_params(FX, FY, CX, CY)

        def route_a(cap=None):
            cands, _, out, pts, offs = m.l2_db_detect_loops_points(curr, args.gap, cand_cap=args.frames, cap=cap, **rule)
            i = m.launch_info()
            return cands, out, pts, offs, (i.kernel_ms, i.aux_kernel_ms)

        def route_b(cap=None):
            cands, _, res, out, pts, mask, offs = m.epi_db_detect_loops(curr, args.gap, ep, cand_cap=args.frames, cap=cap, **rule)
            i = m.launch_info()
            return cands, out, pts, offs, (i.kernel_ms, i.aux_kernel_ms), res, mask

        a, b = route_a(), route_b()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and \
            (a[3] == b[3]).all(), "routes differ"
        total, res = len(a[1]), b[5]
        loops = sum(pkg.capi.epi_loop_test(r, ep) for r in res)
        lines.append(f"online: slot {curr} against {curr - args.gap + 1} slots, {len(a[0])} candidates, {total} survivors in all; candidates, records, "
                     f"point pairs and offsets equal byte for byte; inliers per candidate min {res['n_inliers'].min()} max "
                     f"{res['n_inliers'].max()}, {loops} pass lcm_epi_loop_test; iters {ep.iters}")
        t = {"a": {"kernel": [], "aux": [], "wall": []}, "b": {"kernel": [], "aux": [], "wall": []}}
        for _ in range(args.warmup):
            route_a(total), route_b(total)
        for _ in range(args.calls):
            for name, call in (("a", route_a), ("b", route_b)):
                t0 = time.perf_counter()
                r = call(total)
                t[name]["wall"].append((time.perf_counter() - t0) * 1e3)
                t[name]["kernel"].append(r[4][0])
                t[name]["aux"].append(r[4][1])
        for name, label in (("a", "online (a) lcm_l2_db_detect_loops_points"), ("b", "online (b) lcm_epi_db_detect_loops")):
            r = t[name]
            lines.append(f"{label:<44} kernel_ms {mmm(r['kernel'])} | aux_kernel_ms {mmm(r['aux'])} | wall_ms {mmm(r['wall'])}")
        wa, wb = statistics.median(t["a"]["wall"]), statistics.median(t["b"]["wall"])
        xa, xb = statistics.median(t["a"]["aux"]), statistics.median(t["b"]["aux"])
        lines.append(f"verification adds {wb - wa:.3f} ms of wall time (median to median) and {xb - xa:.3f} ms of aux_kernel_ms to a candidate search of "
                     f"{wa:.3f} ms: {'less' if wb - wa < wa else 'NOT less'} than the search itself costs")

        for iters in (256, 1024, 4096):
            e = pkg.capi.default_epi_params(FX, FY, CX, CY, iters=iters)
            ks, ws = [], []
            for k in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                m.epi_verify_pairs(a[2], a[3], e)
                w = (time.perf_counter() - t0) * 1e3
                if k >= args.warmup:
                    ks.append(m.launch_info().kernel_ms)
                    ws.append(w)
            lines.append(f"kernels: lcm_epi_verify_pairs, {len(a[0])} pairs, {total} point pairs, iters {iters:5d}: kernel_ms (solve + score + mask) "
                         f"{mmm(ks)} | wall_ms {mmm(ws)}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()

"""Times the pose recovery and the choice of the best loop on the device (lcm_pose_db_detect_loops; lcm_pose.hip) against
the loop verification it extends (lcm_epi_db_detect_loops), in one process and one run.

Frames: tools/epi_time.py's (--frames stored frames x --rows rows of uniform random bytes, --shared rows of every frame copies
of one pool with noise of -3..3 per byte, numpy default_rng(41)), with keypoints from a two-view scene (K = 700, 700, 320,
240); a fifth of the pool rows get uniformly random train-side coordinates instead.

  online   the last stored frame against the slots [0, last - gap] (query == NULL form, min_matches = 200):
           (b) lcm_epi_db_detect_loops: the yardstick, unchanged code;
           (c) lcm_pose_db_detect_loops (the same, then k_pose_recover on the device's records, matrices and mask, and
               lcm_pose_best on the host).
  kernel   lcm_pose_recover_pairs alone on (b)'s point pairs, matrices and masks: kernel_ms is k_pose_recover's own time.

Everything the two routes share is compared byte for byte first, then: warm-up calls of both routes and --calls timed calls
ALTERNATING between them; kernel_ms, aux_kernel_ms and wall time as median (min - max).  No CPU recoverPose is timed.

    python tools/pose_time.py            # writes profiles/pose_time.txt and prints it
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ratio", type=float, default=0.7)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--shared", type=int, default=300)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--gap", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_time.txt"))
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
    lines = [f"pose_time: {args.frames} stored frames x {args.rows} rows, {args.shared} shared rows per frame ({args.shared - args.shared // 5} true "
             f"correspondences of a two-view scene, {args.shared // 5} false), ratio {args.ratio}, {args.calls} timed calls per route after "
             f"{args.warmup} warm-up calls, the two routes alternating"]
    rule = dict(ratio=args.ratio, min_rows=1, min_matches=200)

    with pkg.Matcher() as m:
        for k in ("LCM_TUNE_L2_CHUNK", "LCM_TUNE_L2_COUNT_CHUNK"):
            os.environ.pop(k, None)
        for f, kp in zip(frames, kps):
            m.l2_db_append_kp(f, kp)
        ep = pkg.capi.default_epi_params(FX, FY, CX, CY)

        def route_b(cap=None):
            cands, _, res, out, pts, mask, offs = m.epi_db_detect_loops(curr, args.gap, ep, cand_cap=args.frames, cap=cap, **rule)
            i = m.launch_info()
            return (cands, res, out, pts, mask, offs), (i.kernel_ms, i.aux_kernel_ms, i.launches)

        def route_c(cap=None):
            cands, _, res, pres, out, pts, mask, pmask, offs, best = m.pose_db_detect_loops(curr, args.gap, ep, cand_cap=args.frames, cap=cap, **rule)
            i = m.launch_info()
            return (cands, res, out, pts, mask, offs), (i.kernel_ms, i.aux_kernel_ms, i.launches), pres, pmask, best

        b, c = route_b(), route_c()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(b[0], c[0])), "routes differ"
        cands, res, out, pts, mask, offs = b[0]
        total, pres, best = len(out), c[2], c[4]
        passing = sum(pkg.capi.pose_loop_test(r, q, ep) for r, q in zip(res, pres))
        lines.append(f"online: slot {curr} against {curr - args.gap + 1} slots, {len(cands)} candidates, {total} survivors in all; candidates, RANSAC "
                     f"results, records, point pairs, masks and offsets equal byte for byte; launches {b[1][2]} -> {c[1][2]}; iters {ep.iters}; "
                     f"inliers per candidate min {res['n_inliers'].min()} max {res['n_inliers'].max()}, in front min {pres['n_good'].min()} max "
                     f"{pres['n_good'].max()}, {passing} pass lcm_pose_loop_test, best loop = candidate {best} (slot "
                     f"{int(cands[best]['matched_frame_id']) if best >= 0 else -1})")
        t = {"b": {"kernel": [], "aux": [], "wall": []}, "c": {"kernel": [], "aux": [], "wall": []}}
        for _ in range(args.warmup):
            route_b(total), route_c(total)
        for _ in range(args.calls):
            for name, call in (("b", route_b), ("c", route_c)):
                t0 = time.perf_counter()
                r = call(total)
                t[name]["wall"].append((time.perf_counter() - t0) * 1e3)
                t[name]["kernel"].append(r[1][0])
                t[name]["aux"].append(r[1][1])
        for name, label in (("b", "online (b) lcm_epi_db_detect_loops"), ("c", "online (c) lcm_pose_db_detect_loops")):
            r = t[name]
            lines.append(f"{label:<44} kernel_ms {mmm(r['kernel'])} | aux_kernel_ms {mmm(r['aux'])} | wall_ms {mmm(r['wall'])}")
        wb, wc = statistics.median(t["b"]["wall"]), statistics.median(t["c"]["wall"])
        xb, xc = statistics.median(t["b"]["aux"]), statistics.median(t["c"]["aux"])
        lines.append(f"the pose stage adds {wc - wb:.3f} ms of wall time (median to median) and {xc - xb:.3f} ms of aux_kernel_ms to a verification of "
                     f"{wb:.3f} ms (expected: one launch's latency, below the 0.136 ms the three RANSAC kernels added)")

        ks, ws = [], []
        for k in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            m.pose_recover_pairs(pts, offs, res["E"], ep, None, mask)
            w = (time.perf_counter() - t0) * 1e3
            if k >= args.warmup:
                ks.append(m.launch_info().kernel_ms)
                ws.append(w)
        lines.append(f"kernel: lcm_pose_recover_pairs, {len(cands)} pairs, {total} point pairs: kernel_ms (k_pose_recover) {mmm(ks)} | wall_ms {mmm(ws)}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()

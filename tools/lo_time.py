"""Times the RANSAC's local optimisation on the device (lcm_lo_db_detect_loops; lcm_lo.hip) against the loop verification
and pose recovery it sits between (lcm_pose_db_detect_loops), in one process and one run.

Frames: tools/pose_time.py's (--frames stored frames x --rows rows of uniform random bytes, --shared rows of every frame
copies of one pool with noise of -3..3 per byte, numpy default_rng(41)), with keypoints from a two-view scene (K = 700, 700,
320, 240); a fifth of the pool rows get uniformly random train-side coordinates instead; the others carry Gaussian keypoint
noise of --sigma pixels (0.3; 0 gives pose_time's noise-free scene).

  online   the last stored frame against the slots [0, last - gap] (query == NULL form, min_matches = 200):
           (c) lcm_pose_db_detect_loops: the yardstick, unchanged code;
           (d) lcm_lo_db_detect_loops (the same with k_lo_select and k_lo_refine between the RANSAC and k_pose_recover).
  kernel   lcm_epi_verify_pairs and lcm_lo_verify_pairs on (c)'s point pairs: kernel_ms is the RANSAC's three kernels, and
           those plus the optimisation's two; lcm_pose_recover_pairs beside them.

Everything the two routes share is compared byte for byte first, then: warm-up calls of both routes and --calls timed calls
ALTERNATING between them; kernel_ms, aux_kernel_ms and wall time as median (min - max).

    python tools/lo_time.py            # writes profiles/lo_time.txt and prints it
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
    ap.add_argument("--sigma", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lo_time.txt"))
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
    if args.sigma > 0:                           # drawn last: the frames above are pose_time's
        for kp in kps:
            kp += rng.normal(0.0, args.sigma, kp.shape).astype(np.float32)
    lines = [f"lo_time: {args.frames} stored frames x {args.rows} rows, {args.shared} shared rows per frame ({args.shared - args.shared // 5} true "
             f"correspondences of a two-view scene, {args.shared // 5} false), keypoint noise sigma {args.sigma} px, ratio {args.ratio}, "
             f"{args.calls} timed calls per route after {args.warmup} warm-up calls, the two routes alternating"]
    rule = dict(ratio=args.ratio, min_rows=1, min_matches=200)

    with pkg.Matcher() as m:
        for k in ("LCM_TUNE_L2_CHUNK", "LCM_TUNE_L2_COUNT_CHUNK"):
            os.environ.pop(k, None)
        for f, kp in zip(frames, kps):
            m.l2_db_append_kp(f, kp)
        ep = pkg.capi.default_epi_params(FX, FY, CX, CY)

        def route_c(cap=None):
            cands, _, res, pres, out, pts, mask, pmask, offs, best = m.pose_db_detect_loops(curr, args.gap, ep, cand_cap=args.frames, cap=cap, **rule)
            i = m.launch_info()
            return (cands, out, pts, offs), (i.kernel_ms, i.aux_kernel_ms, i.launches), res, pres, mask, best

        def route_d(cap=None):
            cands, _, res, info, pres, out, pts, mask, pmask, offs, best = m.lo_db_detect_loops(curr, args.gap, ep, cand_cap=args.frames, cap=cap, **rule)
            i = m.launch_info()
            return (cands, out, pts, offs), (i.kernel_ms, i.aux_kernel_ms, i.launches), res, pres, mask, best, info

        c, d = route_c(), route_d()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(c[0], d[0])), "routes differ"
        cands, out, pts, offs = c[0]
        total = len(out)
        assert (d[6]["n_inliers_ransac"] == c[2]["n_inliers"]).all() and (d[2]["n_inliers"] >= c[2]["n_inliers"]).all()
        pass_c = sum(pkg.capi.pose_loop_test(r, q, ep) for r, q in zip(c[2], c[3]))
        pass_d = sum(pkg.capi.pose_loop_test(r, q, ep) for r, q in zip(d[2], d[3]))
        lines.append(f"online: slot {curr} against {curr - args.gap + 1} slots, {len(cands)} candidates, {total} survivors in all; candidates, "
                     f"records, point pairs and offsets equal byte for byte, the RANSAC's counts equal; launches {c[1][2]} -> {d[1][2]}; iters "
                     f"{ep.iters}; inliers per candidate min {c[2]['n_inliers'].min()} max {c[2]['n_inliers'].max()} -> min "
                     f"{d[2]['n_inliers'].min()} max {d[2]['n_inliers'].max()}, {int((d[6]['round'] >= 0).sum())} candidates improved; "
                     f"{pass_c} -> {pass_d} pass lcm_pose_loop_test; best loop = candidate {c[5]} -> {d[5]}")
        t = {"c": {"kernel": [], "aux": [], "wall": []}, "d": {"kernel": [], "aux": [], "wall": []}}
        for _ in range(args.warmup):
            route_c(total), route_d(total)
        for _ in range(args.calls):
            for name, call in (("c", route_c), ("d", route_d)):
                t0 = time.perf_counter()
                r = call(total)
                t[name]["wall"].append((time.perf_counter() - t0) * 1e3)
                t[name]["kernel"].append(r[1][0])
                t[name]["aux"].append(r[1][1])
        for name, label in (("c", "online (c) lcm_pose_db_detect_loops"), ("d", "online (d) lcm_lo_db_detect_loops")):
            r = t[name]
            lines.append(f"{label:<44} kernel_ms {mmm(r['kernel'])} | aux_kernel_ms {mmm(r['aux'])} | wall_ms {mmm(r['wall'])}")
        wc, wd = statistics.median(t["c"]["wall"]), statistics.median(t["d"]["wall"])
        xc, xd = statistics.median(t["c"]["aux"]), statistics.median(t["d"]["aux"])
        lines.append(f"the optimisation adds {wd - wc:.3f} ms of wall time (median to median) and {xd - xc:.3f} ms of aux_kernel_ms to a search of "
                     f"{wc:.3f} ms")

        ke, kl, kp_ = [], [], []
        for k in range(args.warmup + args.calls):
            res, _ = m.epi_verify_pairs(pts, offs, ep)
            e_ms = m.launch_info().kernel_ms
            res2, _, mask2 = m.lo_verify_pairs(pts, offs, ep)
            l_ms = m.launch_info().kernel_ms
            m.pose_recover_pairs(pts, offs, res2["E"], ep, None, mask2)
            p_ms = m.launch_info().kernel_ms
            if k >= args.warmup:
                ke.append(e_ms), kl.append(l_ms), kp_.append(p_ms)
        lines.append(f"kernel: {len(cands)} pairs, {total} point pairs: kernel_ms lcm_epi_verify_pairs (the RANSAC's three kernels) {mmm(ke)} | "
                     f"lcm_lo_verify_pairs (those and k_lo_select, k_lo_refine) {mmm(kl)} | lcm_pose_recover_pairs {mmm(kp_)}")
        lines.append(f"the optimisation's two kernels: {statistics.median(kl) - statistics.median(ke):.3f} ms (median to median)")
        # where the time goes: the rounds are alike, so their number splits a round's cost from the rest; half the records of
        # every pair split a round into its passes over the records and its eigen step
        half = np.concatenate([pts[int(offs[p]):int(offs[p]) + (int(offs[p + 1]) - int(offs[p])) // 2] for p in range(len(cands))])
        half_offs = np.concatenate([[0], np.cumsum([(int(offs[p + 1]) - int(offs[p])) // 2 for p in range(len(cands))])]).astype(np.uintp)
        for label, pp, oo in (("all records", pts, offs), ("half the records", half, half_offs)):
            per = []
            for rounds in (1, 2, 4):
                lp = pkg.capi.default_lo_params(mult=(3.0, 2.0, 1.5, 1.0)[:rounds] if rounds < 4 else None)
                ks = []
                for k in range(args.warmup + args.calls):
                    m.lo_verify_pairs(pp, oo, ep, lp)
                    if k >= args.warmup:
                        ks.append(m.launch_info().kernel_ms)
                per.append(statistics.median(ks))
            lines.append(f"rounds, {label}: lcm_lo_verify_pairs kernel_ms at 1 / 2 / 4 rounds {per[0]:.3f} / {per[1]:.3f} / {per[2]:.3f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()

"""Times the loop correspondences of the SIFT keyframe store made on the device (lcm_l2_db_match_points,
lcm_l2_db_detect_loops_points; lcm_l2_emit.hip) against the host-filter route they replace, in one process and one run.

Frames: --frames stored frames x --rows rows of uniform random bytes; --shared of every frame's rows, at positions of the
frame's own, are copies of one pool of random rows with noise of -3..3 per byte (numpy default_rng(41)).  A shared row's
nearest neighbour in any other frame is its copy there (D about 1000) and the second one a random row (D about 1.4 M): it
passes the ratio test, the other rows do not.  A frame's keypoints are (slot * 65536 + row, row / 8) as float32 values.

  bulk     all pairs with curr - past >= --gap (528 pairs):
           (a) lcm_l2_db_match_pairs_ratio (16 bytes per query row come back, the ratio test runs on the host, twice) plus a
               numpy gather of the point pairs;
           (b) lcm_l2_db_match_points.
  online   the last stored frame against the slots [0, last - gap] (query == NULL form, min_matches = 200):
           (a) lcm_l2_db_detect_loops, then lcm_l2_db_match_pairs_ratio on its candidates, plus the numpy gather;
           (b) lcm_l2_db_detect_loops_points.

Per case the outputs of the two routes are compared byte for byte, then: warm-up calls of both routes and --calls timed
calls ALTERNATING between them; kernel_ms (device events around the score / count kernels, summed over the route's calls),
aux_kernel_ms (the count / scan / list kernels of (b)) and the route's wall time as median (min - max).

    python tools/l2_points_time.py            # writes profiles/l2_points_time.txt and prints it
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def measure_alternating(routes, warmup, calls):
    """routes: {name: call -> (kernel_ms, aux_kernel_ms)}.  Returns {name: {"kernel": [...], "aux": [...], "wall": [...]}}."""
    out = {name: {"kernel": [], "aux": [], "wall": []} for name in routes}
    for _ in range(warmup):
        for call in routes.values():
            call()
    for _ in range(calls):
        for name, call in routes.items():
            t0 = time.perf_counter()
            k, a = call()
            out[name]["wall"].append((time.perf_counter() - t0) * 1e3)
            out[name]["kernel"].append(k)
            out[name]["aux"].append(a)
    return out


def mmm(v):
    return f"{statistics.median(v):8.3f} ({min(v):8.3f} - {max(v):8.3f})"


def line(name, r):
    return f"{name:<58} kernel_ms {mmm(r['kernel'])} | aux_kernel_ms {mmm(r['aux'])} | wall_ms {mmm(r['wall'])}"


def verdict(tag, a, b):
    wa, wb = statistics.median(a["wall"]), statistics.median(b["wall"])
    kb = statistics.median(b["kernel"]) + statistics.median(b["aux"])
    return [f"{tag}: (b) wall median {wb:.3f} ms {'<' if wb < wa else '>='} (a) wall median {wa:.3f} ms ({wa / wb:.2f}x)",
            f"{tag}: (b) wall median {wb:.3f} ms is {wb / kb:.2f}x its kernel_ms + aux_kernel_ms medians ({kb:.3f} ms)"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ratio", type=float, default=0.7)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--shared", type=int, default=300)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--gap", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l2_points_time.txt"))
    args = ap.parse_args()

    import numpy as np
    pkg = entry.load_package()
    rng = np.random.default_rng(41)
    pool = rng.integers(0, 256, (args.shared, 128), dtype=np.uint8)
    frames, kps = [], []
    for f in range(args.frames):
        rows = rng.integers(0, 256, (args.rows, 128), dtype=np.uint8)
        at = rng.permutation(args.rows)[: args.shared]
        rows[at] = np.clip(pool.astype(np.int16) + rng.integers(-3, 4, pool.shape), 0, 255).astype(np.uint8)
        frames.append(rows)
        r = np.arange(args.rows, dtype=np.float32)
        kps.append(np.stack([np.float32(f * 65536) + r, r / np.float32(8)], axis=1))
    pairs = [(c, p) for c in range(args.frames) for p in range(args.frames) if c - p >= args.gap]
    lines = [f"l2_points_time: {args.frames} stored frames x {args.rows} rows, {args.shared} shared rows per frame (pool + noise -3..3, "
             f"default_rng(41)), ratio {args.ratio}, {args.calls} timed calls per route after {args.warmup} warm-up calls, the two routes of "
             f"a case alternating"]

    def gather(out, offs, pr):
        pts = np.empty((len(out), 4), np.float32)
        for k, (q, t) in enumerate(pr):
            rec = out[int(offs[k]): int(offs[k + 1])]
            pts[int(offs[k]): int(offs[k + 1]), :2] = kps[q][rec["query_idx"]]
            pts[int(offs[k]): int(offs[k + 1]), 2:] = kps[t][rec["train_idx"]]
        return pts

    with pkg.Matcher() as m:
        for k in ("LCM_TUNE_L2_CHUNK", "LCM_TUNE_L2_COUNT_CHUNK"):
            os.environ.pop(k, None)
        for f, kp in zip(frames, kps):
            m.l2_db_append_kp(f, kp)
        info = m.l2_db_info()
        lines.append(f"store: {info.tiles_used} tiles used, {info.tiles_reserved} reserved, {info.device_bytes / 2**20:.1f} MiB on the device "
                     f"(the points arena: {info.tiles_reserved * 256 / 2**20:.1f} MiB)")

        # ---- bulk
        def bulk_a(cap=None):
            lists, offs = m.l2_db_match_pairs_ratio(pairs, args.ratio, cap=cap)
            i = m.launch_info()
            out = np.concatenate(lists)
            return out, gather(out, offs, pairs), offs, (i.kernel_ms, i.aux_kernel_ms)

        def bulk_b(cap=None):
            out, pts, offs = m.l2_db_match_points(pairs, args.ratio, cap=cap)
            i = m.launch_info()
            return out, pts, offs, (i.kernel_ms, i.aux_kernel_ms)

        a, b = bulk_a(), bulk_b()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and (a[2] == b[2]).all(), "bulk: routes differ"
        total = len(a[0])
        per = np.diff(a[2].astype(np.int64))
        lines.append(f"bulk: {len(pairs)} pairs (curr - past >= {args.gap}), {total} survivors in all (per pair min {per.min()} max {per.max()}), "
                     f"records, point pairs and offsets equal byte for byte; (a) downloads {16 * args.rows * len(pairs)} bytes, "
                     f"(b) {8 * (len(pairs) + 1) + 32 * total}")
        r = measure_alternating({"a": lambda: bulk_a(total)[3], "b": lambda: bulk_b(total)[3]}, args.warmup, args.calls)
        lines.append(line("bulk (a) lcm_l2_db_match_pairs_ratio + numpy gather", r["a"]))
        lines.append(line("bulk (b) lcm_l2_db_match_points", r["b"]))
        lines += verdict("bulk", r["a"], r["b"])

        # ---- online: the last stored frame against the slots [0, last - gap]
        curr = args.frames - 1
        rule = dict(ratio=args.ratio, min_rows=1, min_matches=200)

        def online_a(cap=None):
            cands, _ = m.l2_db_detect_loops(curr, args.gap, cap=args.frames, **rule)
            i = m.launch_info()
            pr = [(curr, int(p)) for p in cands["matched_frame_id"]]
            lists, offs = m.l2_db_match_pairs_ratio(pr, args.ratio, cap=cap)
            j = m.launch_info()
            out = np.concatenate(lists) if lists else np.zeros(0, pkg.capi.DMATCH_DTYPE)
            return cands, out, gather(out, offs, pr), offs, (i.kernel_ms + j.kernel_ms, i.aux_kernel_ms + j.aux_kernel_ms)

        def online_b(cap=None):
            cands, _, out, pts, offs = m.l2_db_detect_loops_points(curr, args.gap, cand_cap=args.frames, cap=cap, **rule)
            i = m.launch_info()
            return cands, out, pts, offs, (i.kernel_ms, i.aux_kernel_ms)

        a, b = online_a(), online_b()
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and \
            (a[3] == b[3]).all(), "online: routes differ"
        total = len(a[1])
        lines.append(f"online: slot {curr} against {curr - args.gap + 1} slots, {len(a[0])} candidates, {total} survivors in all, candidates, "
                     f"records, point pairs and offsets equal byte for byte")
        r = measure_alternating({"a": lambda: online_a(total)[4], "b": lambda: online_b(total)[4]}, args.warmup, args.calls)
        lines.append(line("online (a) detect_loops + match_pairs_ratio + numpy gather", r["a"]))
        lines.append(line("online (b) lcm_l2_db_detect_loops_points", r["b"]))
        lines += verdict("online", r["a"], r["b"])
        lines.append("online (b): kernel_ms is its score kernel's alone (the count kernel of the candidate search ran before it); (a)'s sums both calls'")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()

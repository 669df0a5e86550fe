"""Times the loop search over the SIFT keyframe store (lcm_l2_db_detect_loops, lcm_l2_db_loop_search; lcm_l2_store.hip)
against the host-matrix calls it replaces, in one process and one run, on tools/l2_count_time.py's frames: 64 frames x 4000
rows plus one query frame.

  online   one new keyframe against the 64 stored ones (64 pairs, 1.0 G distances):
           (a) lcm_score_pairs_ratio_l2 over the 64 (query, stored) pairs with all 65 host matrices: every call uploads
               and packs all of them;
           (b) lcm_l2_db_detect_loops with the query's host rows: uploads and packs the query alone.
  bulk     all pairs with curr - past >= 32 (528 pairs, 8.4 G distances):
           (a) lcm_loop_search_ratio_l2 over the 64 host matrices;  (b) lcm_l2_db_loop_search over the stored ones.

Per case: warm-up calls of both routes, then --calls timed calls ALTERNATING between the two routes; the median, minimum
and maximum of kernel_ms (device events around the count kernel) and of the call's wall time.  The counts of the two
routes are compared pair for pair before anything is timed.  The last lines say whether (b)'s wall time is below (a)'s
and whether (b)'s median kernel_ms lies within (a)'s own min-max spread.

    python tools/l2_store_time.py            # writes profiles/l2_store_time.txt and prints it
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def measure_alternating(routes, info, warmup, calls):
    """routes: {name: call}.  Returns {name: {"kernel": [...], "wall": [...], "workgroups", "distances"}}."""
    out = {name: {"kernel": [], "wall": []} for name in routes}
    for _ in range(warmup):
        for call in routes.values():
            call()
    for _ in range(calls):
        for name, call in routes.items():
            t0 = time.perf_counter()
            call()
            out[name]["wall"].append((time.perf_counter() - t0) * 1e3)
            i = info()
            out[name]["kernel"].append(i.kernel_ms)
            out[name]["workgroups"], out[name]["distances"] = i.workgroups, i.distances
    return out


def line(name, r):
    k, w = r["kernel"], r["wall"]
    med = statistics.median(k)
    return (f"{name:<52} kernel_ms median {med:8.3f} min {min(k):8.3f} max {max(k):8.3f} | wall_ms median "
            f"{statistics.median(w):8.3f} min {min(w):8.3f} max {max(w):8.3f} | workgroups {r['workgroups']:6d} | "
            f"{r['distances'] / (med * 1e-3) / 1e12:6.2f} T distances/s")


def verdicts(tag, a, b):
    wa, wb = statistics.median(a["wall"]), statistics.median(b["wall"])
    kb = statistics.median(b["kernel"])
    lo, hi = min(a["kernel"]), max(a["kernel"])
    return [f"{tag}: (b) wall median {wb:.3f} ms {'<' if wb < wa else '>='} (a) wall median {wa:.3f} ms ({wa / wb:.2f}x)",
            f"{tag}: (b) kernel_ms median {kb:.3f} {'inside' if lo <= kb <= hi else 'OUTSIDE'} (a)'s min-max [{lo:.3f}, {hi:.3f}]"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ratio", type=float, default=0.7)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--gap", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l2_store_time.txt"))
    args = ap.parse_args()

    import numpy as np
    pkg = entry.load_package()
    rng = np.random.default_rng(31)
    n_all = args.frames + 1
    frames = [rng.integers(0, 256, (args.rows, 128), dtype=np.uint8) for _ in range(n_all)]
    for f in range(1, n_all):                            # half of every frame's rows are near copies of the previous frame's
        n = args.rows // 2
        frames[f][:n] = np.clip(frames[f - 1][:n].astype(np.int16) + rng.integers(-20, 21, (n, 128)), 0, 255).astype(np.uint8)
    stored, query = frames[:args.frames], frames[args.frames]
    online_pairs = [(args.frames, p) for p in range(args.frames)]
    n_bulk = sum(1 for c in range(args.frames) for p in range(args.frames) if c - p >= args.gap)
    every = dict(ratio=args.ratio, min_rows=1, min_matches=0)      # every scored pair comes back as a candidate
    lines = [f"l2_store_time: {args.frames} stored frames x {args.rows} rows + one query frame, ratio {args.ratio}, {args.calls} timed calls "
             f"per route after {args.warmup} warm-up calls, the two routes of a case alternating"]

    with pkg.Matcher() as m:
        os.environ.pop("LCM_TUNE_L2_COUNT_CHUNK", None)
        t0 = time.perf_counter()
        for f in stored:
            m.l2_db_append(f)
        append_ms = (time.perf_counter() - t0) * 1e3
        info = m.l2_db_info()
        lines.append(f"append: {args.frames} frames in {append_ms:.1f} ms ({append_ms / args.frames:.3f} ms per frame, upload + pack + wait); "
                     f"{info.tiles_used} tiles used, {info.tiles_reserved} reserved, {info.device_bytes / 2**20:.1f} MiB on the device")

        # ---- online: one keyframe against the store
        a = m.score_pairs_ratio_l2(frames, online_pairs, args.ratio)
        b, n_pairs = m.l2_db_detect_loops(args.frames, 1, query=query, cap=args.frames, **every)
        assert n_pairs == len(online_pairs) == len(b)
        assert (b["matched_frame_id"] == np.arange(args.frames)).all() and (b["num_matches"] == a["good_count"]).all(), "online: store != host matrices"
        lines.append(f"online: {len(online_pairs)} pairs, counts equal pair for pair (min {int(a['good_count'].min())} max {int(a['good_count'].max())}); "
                     f"tables uploaded by (b): {m.l2_db_info().table_bytes} bytes")
        r = measure_alternating({"a": lambda: m.score_pairs_ratio_l2(frames, online_pairs, args.ratio),
                                 "b": lambda: m.l2_db_detect_loops(args.frames, 1, query=query, cap=args.frames, **every)},
                                m.launch_info, args.warmup, args.calls)
        lines.append(line("online (a) lcm_score_pairs_ratio_l2, 65 host matrices", r["a"]))
        lines.append(line("online (b) lcm_l2_db_detect_loops, host query", r["b"]))
        lines += verdicts("online", r["a"], r["b"])

        # ---- bulk: the 528-pair set
        a, na = m.loop_search_ratio_l2(stored, args.gap, cap=n_bulk, **every)
        b, nb = m.l2_db_loop_search(args.gap, cap=n_bulk, **every)
        assert na == nb == n_bulk == len(a) == len(b) and a.tobytes() == b.tobytes(), "bulk: store != host matrices"
        lines.append(f"bulk: {n_bulk} pairs (curr - past >= {args.gap}), candidates equal byte for byte")
        store_tab = m.l2_db_info().table_bytes
        r = measure_alternating({"a": lambda: m.loop_search_ratio_l2(stored, args.gap, cap=n_bulk, **every),
                                 "b": lambda: m.l2_db_loop_search(args.gap, cap=n_bulk, **every)},
                                m.launch_info, args.warmup, args.calls)
        lines.append(line("bulk (a) lcm_loop_search_ratio_l2, 64 host matrices", r["a"]))
        lines.append(line("bulk (b) lcm_l2_db_loop_search", r["b"]))
        lines += verdicts("bulk", r["a"], r["b"])
        lines.append(f"bulk: work tables uploaded per call: (a) {32 * r['a']['workgroups']} bytes of items, (b) {store_tab} bytes of runs and slots")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()

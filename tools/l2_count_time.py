"""Times the ratio-test count per pair on SIFT rows (lcm_score_pairs_ratio_l2, lcm_l2_count.hip) against the list call it
replaces in the loop search (lcm_match_pairs_ratio_l2), in one process and one run, on tools/l2_time.py's shape: 64 frames
x 4000 rows, all pairs with curr - past >= 32 (528 pairs, 8.4 G distances).

  (a) the list call as it stands: kernel_ms (device events around k_l2_score; its fold, rescan and download come after
      them) and the call's wall time;
  (b) the count call with the chunk pinned to 128, to 256 and chosen by the library: kernel_ms (events around k_l2_count)
      and wall time;
  one more line for a single 4000 x 4000 pair, the call that does not fill the chip.

Per case: warm-up calls, then the median, minimum and maximum over --calls repetitions.  The counts of (b) are compared with
the list call's offsets before anything is timed.

    python tools/l2_count_time.py            # writes profiles/l2_count_time.txt and prints it
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402


def measure(call, info, warmup, calls):
    for _ in range(warmup):
        call()
    kernel, wall = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        kernel.append(info().kernel_ms)
    i = info()
    return {"kernel": kernel, "wall": wall, "workgroups": i.workgroups, "distances": i.distances}


def line(name, r):
    k, w = r["kernel"], r["wall"]
    med = statistics.median(k)
    return (f"{name:<44} kernel_ms median {med:8.3f} min {min(k):8.3f} max {max(k):8.3f} | wall_ms median "
            f"{statistics.median(w):8.3f} min {min(w):8.3f} max {max(w):8.3f} | workgroups {r['workgroups']:6d} | "
            f"{r['distances'] / (med * 1e-3) / 1e12:6.2f} T distances/s")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ratio", type=float, default=0.7)
    ap.add_argument("--rows", type=int, default=4000)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--gap", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l2_count_time.txt"))
    args = ap.parse_args()

    import numpy as np
    pkg = entry.load_package()
    rng = np.random.default_rng(31)
    frames = [rng.integers(0, 256, (args.rows, 128), dtype=np.uint8) for _ in range(args.frames)]
    for f in range(1, args.frames):                      # half of every frame's rows are near copies of the previous frame's
        n = args.rows // 2
        frames[f][:n] = np.clip(frames[f - 1][:n].astype(np.int16) + rng.integers(-20, 21, (n, 128)), 0, 255).astype(np.uint8)
    pairs = [(c, p) for c in range(args.frames) for p in range(args.frames) if c - p >= args.gap]
    single = [(1, 0)]
    lines = [f"l2_count_time: {args.frames} frames x {args.rows} rows, {len(pairs)} pairs (curr - past >= {args.gap}), ratio {args.ratio}, "
             f"median of {args.calls} calls after {args.warmup} warm-up calls"]

    def pin(chunk, var="LCM_TUNE_L2_COUNT_CHUNK"):
        if chunk == "auto":
            os.environ.pop(var, None)
        else:
            os.environ[var] = chunk

    with pkg.Matcher() as m:
        pin("auto", "LCM_TUNE_L2_CHUNK")
        _, offs = m.match_pairs_ratio_l2(frames, pairs, args.ratio)
        counts = np.diff(np.asarray(offs, np.int64))
        for chunk in ("128", "256", "auto"):
            pin(chunk)
            got = m.score_pairs_ratio_l2(frames, pairs, args.ratio)
            assert (got["good_count"] == counts).all(), f"count call (chunk {chunk}) != list call"
        lines.append(f"survivors per pair: min {int(counts.min())} median {int(np.median(counts))} max {int(counts.max())}; "
                     f"count call == list call's offsets for all {len(pairs)} pairs, all three chunk settings")
        lines.append(line("(a) list call, lcm_match_pairs_ratio_l2",
                          measure(lambda: m.match_pairs_ratio_l2(frames, pairs, args.ratio), m.launch_info, args.warmup, args.calls)))
        for chunk in ("128", "256", "auto"):
            pin(chunk)
            lines.append(line(f"(b) count call, chunk {chunk}",
                              measure(lambda: m.score_pairs_ratio_l2(frames, pairs, args.ratio), m.launch_info, args.warmup, args.calls)))
        pin("auto")
        lines.append(line(f"single pair {args.rows} x {args.rows}, list call",
                          measure(lambda: m.match_pairs_ratio_l2(frames[:2], single, args.ratio), m.launch_info, args.warmup, args.calls)))
        lines.append(line(f"single pair {args.rows} x {args.rows}, count call (auto)",
                          measure(lambda: m.score_pairs_ratio_l2(frames[:2], single, args.ratio), m.launch_info, args.warmup, args.calls)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
